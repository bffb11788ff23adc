"""The direct k-way multilevel driver and the device contraction without a GPU: the new structs have the layout the
Python mirror assumes (against a compiled C probe), the defaults are the documented ones, and the CLI refuses
--kway-direct with the usage text, before any GPU work, wherever DESIGN.md §19 says it does."""
import ctypes
import os
import subprocess

import pytest

from conftest import PKG_DIR, REPO, circuit_path

GKL2 = os.path.join(PKG_DIR, "build", "bin", "gKL2")


def test_struct_layout_matches_python_mirror(ek, tmp_path):
    src = tmp_path / "layout.c"
    src.write_text(
        '#include <stdio.h>\n#include <stddef.h>\n#include "eigkl.h"\n'
        "int main(void) {\n"
        '  printf("%zu %zu %zu\\n", sizeof(ek_contract_opts), sizeof(ek_kway_direct_opts), sizeof(ek_kway_direct_result));\n'
        '  printf("%zu %zu %zu %zu %zu %zu\\n", offsetof(ek_kway_direct_opts, match), offsetof(ek_kway_direct_opts, initial),'
        " offsetof(ek_kway_direct_opts, jet), offsetof(ek_kway_direct_opts, out_dir),"
        " offsetof(ek_kway_direct_result, conn_w_before), offsetof(ek_kway_direct_result, t_match));\n"
        '  printf("%d %d %d\\n", EK_KWAY_DIRECT_HOST_CONTRACT, EK_KWAY_DIRECT_WEIGHTED_LAPLACIAN, EIGKL_ABI_VERSION);\n'
        "  return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-I", os.path.join(REPO, "include"), str(src), "-o", str(exe)])
    a, b, c = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    assert [int(x) for x in a.split()] == [ctypes.sizeof(ek.ContractOpts), ctypes.sizeof(ek.KwayDirectOpts),
                                           ctypes.sizeof(ek.KwayDirectResult)]
    assert [int(x) for x in b.split()] == [ek.KwayDirectOpts.match.offset, ek.KwayDirectOpts.initial.offset,
                                           ek.KwayDirectOpts.jet.offset, ek.KwayDirectOpts.out_dir.offset,
                                           ek.KwayDirectResult.conn_w_before.offset, ek.KwayDirectResult.t_match.offset]
    assert [int(x) for x in c.split()] == [ek.KWAY_DIRECT_HOST_CONTRACT, ek.KWAY_DIRECT_WEIGHTED_LAPLACIAN, 4]
    assert ek.ABI_VERSION == 4  # only new structs: the ABI number stays


def test_defaults(ek):
    c = ek.ContractOpts(7, 7)
    ek.lib.ek_contract_default_opts(ctypes.byref(c))
    assert (c.hash_bits, c.pad) == (64, 0)
    o = ek.KwayDirectOpts()
    ctypes.memset(ctypes.byref(o), 0x5a, ctypes.sizeof(o))
    ek.lib.ek_kway_direct_default_opts(ctypes.byref(o))
    assert (o.k, o.flags, o.imbalance, o.max_levels, o.write_results, o.out_dir) == (2, 0, 0.03, ek.ML_LEVELS, 0, None)
    assert o.coarse_nodes <= 0 and o.match.max_cluster <= 0  # both derived: max(512, 128 k); from W, Lk and coarse_nodes
    m = ek.MatchOpts()
    ek.lib.ek_match_default_opts(ctypes.byref(m))
    assert (o.match.max_net, o.match.max_rounds) == (m.max_net, m.max_rounds)
    i = ek.KwayMlOpts()
    ek.lib.ek_kway_ml_default_opts(ctypes.byref(i))
    assert bytes(o.initial) == bytes(i)
    j = ek.KwayJetOpts()
    ek.lib.ek_kway_jet_default_opts(ctypes.byref(j))
    assert bytes(o.jet) == bytes(j) and (j.patience, j.neg_num, j.neg_den, j.max_iters) == (12, 1, 4, 0)
    ek.lib.ek_kway_direct_default_opts(None)  # a null pointer is ignored
    ek.lib.ek_contract_default_opts(None)


REFUSED = [
    ["--k", "4", "--kway-direct", "0.03", "--kway-multilevel", "0.03"],
    ["--k", "4", "--kway-multilevel", "0.03", "--kway-direct", "0.03"],
    ["--k", "4", "--kway-direct", "0.03", "--refine", "0.03"],
    ["--k", "4", "--kway-direct", "0.03", "--refine-weighted", "0.03"],
    ["--k", "4", "--kway-direct", "0.03", "--refine-jet", "0.03"],
    ["--k", "4", "--kway-direct", "0.03", "--multilevel", "0.03"],
    ["--k", "4", "--kway-direct", "0.03", "--sweep", "0.03"],
    ["--k", "4", "--kway-direct", "0.03", "--fm", "0.03"],
    ["--kway-direct", "0.03"],                  # without --k
    ["--k", "257", "--kway-direct", "0.03"],    # k outside 2..256
    ["--k", "4", "--kway-direct"],              # without a value
    ["--k", "4", "--kway-direct", "-0.01"],
    ["--k", "4", "--kway-direct", "nan"],
    ["--k", "4", "--kway-direct", "inf"],
    ["--k", "4", "--contract-host"],            # --contract-host needs --kway-direct
]


@pytest.mark.parametrize("flags", REFUSED, ids=lambda f: " ".join(f))
def test_cli_refuses_with_the_usage_text(tmp_path, flags):
    r = subprocess.run([GKL2, circuit_path("fract"), "-EIG"] + flags, cwd=tmp_path, capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert "Usage: gKL2 <input_file> -EIG --k <parts> --kway-direct <imbalance>" in r.stdout
    assert not any(ln.startswith("kway-direct:") for ln in r.stdout.splitlines())
    assert "HIP" not in r.stderr and "device" not in r.stderr  # refused before any GPU work
    assert not (tmp_path / "results").exists()


def test_cli_refuses_other_tools_and_a_missing_eig_flag(tmp_path):
    for argv in ([os.path.join(PKG_DIR, "build", "bin", "gKL"), circuit_path("fract"), "-EIG", "--k", "4",
                  "--kway-direct", "0.03"],
                 [GKL2, circuit_path("fract"), "--k", "4", "--kway-direct", "0.03"]):
        r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--kway-direct <imbalance>" in r.stdout
