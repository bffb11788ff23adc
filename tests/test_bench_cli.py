"""bench.py's command line (no GPU): `--full` gates every leg beyond the timed
steps, and `--dump-outputs` writes the last step's outputs as float arrays."""
import ast
import importlib.util
import os

import numpy as np

from conftest import REPO

BENCH = os.path.join(REPO, "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("ek_bench", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_ends_before_the_extra_legs():
    """A plain run returns at `if not args.full:`; every leg that measures more
    than the timed steps (rocprofv3 passes, event-timed step, parity, SpMV
    benches, resident solve, syn10, sub-configs, fresh process, CPU baseline)
    is called only after that line, or under a condition on `args.full` /
    `extras` (which holds args.full)."""
    src = open(BENCH).read()
    tree = ast.parse(src)
    main = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "main")
    gate = next(n for n in main.body if isinstance(n, ast.If) and ast.unparse(n.test) == "not args.full")
    assert isinstance(gate.body[-1], ast.Return)
    extras = next(n for n in ast.walk(main) if isinstance(n, ast.Assign) and ast.unparse(n.targets[0]) == "extras")
    assert ast.unparse(extras.value).startswith("args.full and ")
    parents = {ch: node for node in ast.walk(main) for ch in ast.iter_child_nodes(node)}
    legs = {"rocprof_pass", "headline_parity", "cpu_baseline", "spmv_gather_bench", "spmv_bench", "lanczos_fiedler",
            "kl_run", "spmv_setup_pins", "probe", "generate"}
    seen = set()
    for node in ast.walk(main):
        if not isinstance(node, ast.Call):
            continue
        name = node.func.attr if isinstance(node.func, ast.Attribute) else getattr(node.func, "id", None)
        timed_spmv = name == "step" and any(k.arg == "time_spmv" for k in node.keywords)
        if name not in legs and not timed_spmv:
            continue
        if name == "generate" and node.lineno < gate.lineno and "args.mult" in ast.unparse(node):
            continue  # the headline workload itself, in the untimed setup
        seen.add(name)
        if node.lineno > gate.end_lineno:
            continue
        p, gated = parents.get(node), False
        while p is not None and not gated:
            if isinstance(p, ast.If):
                names = {n.id for n in ast.walk(p.test) if isinstance(n, ast.Name)}
                gated = "extras" in names or "args.full" in ast.unparse(p.test)
            p = parents.get(p)
        assert gated, f"bench.py:{node.lineno}: {name}() runs in a plain run"
    assert legs <= seen, legs - seen  # (the list above still names what the script calls)


def test_dump_outputs_writes_float_arrays(ek, tmp_path):
    bench = _bench()
    log = np.zeros(3, ek.SWAP_DTYPE)
    log["iter"] = [0, 1, 2]
    log["node_left"] = [5, 2 ** 24 + 1, 7]  # a node index float32 could not hold
    log["node_right"] = [1, 2, 3]
    log["gain"] = np.float32([1.5, -0.25, 0.1])
    log["cut"] = np.float32([10.0, 8.5, 8.75])
    res = tmp_path / "results.txt"
    res.write_text("0\t10\t0\n1\t8.5\t1.5\n")

    class Ctx:
        def kl_sides(self, which):
            assert which == 0
            return np.array([0, 1, 1, 0], np.uint8)

    last = {"lambda": 0.03, "median": -1e-3,
            "kl": {"iterations": 3, "initial_cut": 10.0, "best_cut": 8.5, "best_iter": 1, "net_cut_best": 4,
                   "net_cut_final": 5}}
    d = tmp_path / "dump"
    bench.dump_outputs(str(d), Ctx(), last, log, str(res))
    got = {f[:-4]: np.load(d / f) for f in sorted(os.listdir(d))}
    assert sorted(got) == ["results_file", "scalars", "split", "swap_log"]
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert got["swap_log"].shape == (3, 7) and got["swap_log"][1, 1] == 2 ** 24 + 1
    assert np.array_equal(got["swap_log"][:, 5].astype(np.float32), log["gain"])  # fp32 fields kept exactly
    assert np.array_equal(got["split"], [0, 1, 1, 0])
    assert np.array_equal(got["results_file"], [[0, 10, 0], [1, 8.5, 1.5]])
    assert np.array_equal(got["scalars"], [0.03, -1e-3, 3, 10.0, 8.5, 1, 4, 5])
