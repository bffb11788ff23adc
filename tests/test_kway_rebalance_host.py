"""ek_kway_rebalance_host (no GPU): against the plain-Python restatement of the rule
of DESIGN.md §21 on every case, bit for bit, and the promises the rule makes,
each asserted from the logs and the restatement's per-round states."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import rebalance_cases as bc
from conftest import PKG_DIR, REPO, circuit_path


def run_case(ek, name, case):
    h = bc.hypergraph(ek, case)
    ref = bc.reference(name, case)
    want, want_log = ref[0], ref[1]
    part, res, log = bc.run(ek.kway_rebalance_host, h, case)
    assert np.array_equal(log, want_log), (log[:6].tolist(), want_log[:6].tolist())
    assert np.array_equal(part, want), int(np.count_nonzero(part != want))
    bc.check_properties(ek, h, case, ref, part, res, log)
    bc.check_expect(case, part, res, log)
    return part, res, log


@pytest.mark.parametrize("name", list(bc.built_cases()))
def test_host_equals_restatement_built(ek, name):
    run_case(ek, name, bc.built_cases()[name])


@pytest.mark.parametrize("name", list(bc.random_cases()))
def test_host_equals_restatement_random(ek, name):
    part, res, log = run_case(ek, name, bc.random_cases()[name])
    assert res["rounds"] >= 1 and 1 <= res["parts_over_before"] <= 3


def test_the_cases_cover_what_they_are_for(ek):
    cases = bc.all_cases()
    refs = {name: bc.reference(name, c) for name, c in cases.items()}
    logs = {name: r[1] for name, r in refs.items()}
    # a round that evicts fewer than propose, one that moves fewer than it evicts, a run of several rounds, a run that
    # leaves a part over, and one whose weighted connectivity rises
    assert any(np.any(l[:, 1] < l[:, 0]) for l in logs.values())
    assert any(np.any(l[:, 2] < l[:, 1]) for l in logs.values())
    assert any(len(l) >= 3 for l in logs.values())
    assert any(len(l) and l[-1, 3] > 0 for l in logs.values())
    case = cases["random-0"]
    _, res, _ = bc.run(ek.kway_rebalance_host, bc.hypergraph(ek, case), case)
    assert res["connectivity_w"] != res["connectivity_w_before"]
    # k = 256: sources and targets in each of the four mask words
    own, tgt = set(), set()
    for name in ("gain-k256-perm", "gain-k256-edge"):
        for v in np.flatnonzero(refs[name][0] != cases[name]["start"]):
            own.add(int(cases[name]["start"][v]) >> 6)
            tgt.add(int(refs[name][0][v]) >> 6)
    assert len(own) >= 2 and tgt == {0, 1, 2, 3}, (own, tgt)
    # a moved node on no net, and one on 130 nets
    assert any(len(r["moved"]) for r in refs["no-nets"][3])
    # max_rounds = 1 cuts the two-round run after its first round
    assert np.array_equal(logs["max-rounds-1"], logs["accept-two-sources"][:1])


def test_einval_guards(ek):
    case = bc.built_cases()["accept-two-sources"]
    h = bc.hypergraph(ek, case)
    good = case["start"]
    for k in (1, 257, 0):
        with pytest.raises(ek.EKError) as e:
            ek.kway_rebalance_host(h, np.zeros(4, np.int32), k)
        assert e.value.code == ek.EK_EINVAL, k
    for eps in (-0.01, float("inf"), float("nan")):
        with pytest.raises(ek.EKError) as e:
            ek.kway_rebalance_host(h, good, 4, eps)
        assert e.value.code == ek.EK_EINVAL, eps
    bad = good.copy()
    bad[3] = 4
    with pytest.raises(ek.EKError) as e:
        ek.kway_rebalance_host(h, bad, 4)
    assert e.value.code == ek.EK_EINVAL
    with pytest.raises(ek.EKError) as e:
        ek.kway_rebalance_host(h, good, 4, bounds=[1, 1, -1, 10])
    assert e.value.code == ek.EK_EINVAL
    with pytest.raises(ValueError):
        ek.kway_rebalance_host(h, good, 4, bounds=[1, 2, 3])
    with pytest.raises(ValueError):
        ek.kway_rebalance_host(h, good[:-1], 4)
    # max_rounds <= 0 is a value, not an error; and the log-capacity retry gives the whole log
    assert ek.kway_rebalance_host(h, good, 4, bounds=case["bounds"], max_rounds=-1)[1]["rounds"] == 2
    part, res, log = ek.kway_rebalance_host(h, good, 4, bounds=case["bounds"])
    o = ek.KwayRebalanceOpts()
    ek.lib.ek_kway_rebalance_default_opts(ctypes.byref(o))
    o.k = 4
    r, short, out = ek.KwayRebalanceResult(), np.zeros((1, 4), np.int64), good.copy()
    rc = ek.lib.ek_kway_rebalance_host(h._h, ctypes.byref(o), case["bounds"].ctypes.data, out.ctypes.data,
                                       short.ctypes.data, 1, ctypes.byref(r))
    assert rc == 0 and r.rounds == 2 and np.array_equal(short, log[:1]) and np.array_equal(out, part)


def test_symbols_struct_layout_and_abi(ek, tmp_path):
    hdr = open(os.path.join(REPO, "include", "eigkl.h")).read()
    for name in ("ek_kway_rebalance_host", "ek_kway_rebalance", "ek_kway_rebalance_default_opts",
                 "ek_partition_kway_direct_rb", "ek_partition_kway_direct_rb_file"):
        assert re.search(rf"\b{name}\s*\(", hdr) and hasattr(ek.lib, name)
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "eigkl.h"', "int main(void) {",
             '  printf("%d\\n", EIGKL_ABI_VERSION);']
    want = [4]
    for c_name, cls in (("ek_kway_rebalance_result", ek.KwayRebalanceResult),
                        ("ek_kway_rebalance_opts", ek.KwayRebalanceOpts),
                        ("ek_kway_direct_rb_result", ek.KwayDirectRbResult),
                        ("ek_kway_direct_opts", ek.KwayDirectOpts), ("ek_kway_direct_result", ek.KwayDirectResult)):
        fields = [n for n, _ in cls._fields_]
        lines += [f'  printf("%zu\\n", sizeof({c_name}));']
        lines += [f'  printf("%zu\\n", offsetof({c_name}, {n}));' for n in fields]
        want += [ctypes.sizeof(cls)] + [getattr(cls, n).offset for n in fields]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == want
    assert ek.ABI_VERSION == 4 == ek.lib.ek_abi_version()  # new structs only: no existing layout changed
    o = ek.KwayRebalanceOpts()
    ek.lib.ek_kway_rebalance_default_opts(ctypes.byref(o))
    assert (o.k, o.max_rounds, o.imbalance) == (2, 0, 0.03)


def test_rebalance_cli_misuse_prints_usage(tmp_path):
    """Refused while the arguments are read: no GPU work, no results file.  --rebalance needs --kway-direct;
    --rebalance-to follows --kway-multilevel only and takes a finite imbalance >= 0."""
    tool = os.path.join(PKG_DIR, "build", "bin", "gKL2")
    ml = ("-EIG", "--k", "4", "--kway-multilevel", "0.03")
    for args, word in ((("-EIG", "--k", "4", "--rebalance"), "--kway-direct"),
                       (("-EIG", "--rebalance"), "--kway-direct"),
                       ((*ml, "--rebalance"), "--kway-direct"),
                       (("-EIG", "--k", "4", "--kway-direct", "0.03", "--rebalance", "--rebalance-to", "0.01"),
                        "--kway-direct"),
                       (("-EIG", "--k", "4", "--rebalance-to", "0.01"), "--kway-multilevel"),
                       (("-EIG", "--k", "4", "--multilevel", "0.03", "--rebalance-to", "0.01"), "--kway-multilevel"),
                       ((*ml, "--rebalance-to"), "--kway-multilevel"),
                       ((*ml, "--rebalance-to", "-0.1"), "--kway-multilevel"),
                       ((*ml, "--rebalance-to", "nan"), "--kway-multilevel"),
                       ((*ml, "--rebalance-to", "inf"), "--kway-multilevel"),
                       ((*ml, "--rebalance-to", "x"), "--kway-multilevel"),
                       ((*ml, "--rebalance-to", "0.01", "--refine-weighted", "0.05"), "--kway-multilevel")):
        r = subprocess.run([tool, circuit_path("fract"), *args], cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "Usage: gKL2" in r.stdout and word in r.stdout, (args, r.stdout)
        assert "--rebalance" in r.stdout, args
        assert not (tmp_path / "results" / "fract.hgr.part.4").exists()
