"""The KL swap loops on the shape cases of kl_cases.py (chunk, list, item-count,
row-length and weight-code edges; test_kl_cases_host.py proves each case holds
its shape), in every loop form kl_loop can dispatch, against the numpy
reference.  Every comparison is equality of bits or integers.

kl_sides: 0 is the initial partition, 1 the best prefix, 2 the final state;
all three are held to the reference.

Every form takes every case (kl_loop: the LDS forms fit up to fix-65's 65
chunks, EK_KL_GBITS only needs KLDev::locked, which ek_kl_graph_setup always
allocates), so no (form, case) pair is left out for the dispatch's sake; the
two long-list cases run in three forms only, to keep the suite short."""
import numpy as np
import pytest

import kl_cases as kc
from conftest import swap_fields_equal

pytestmark = pytest.mark.gpu

FORMS = {
    "default": {},                                   # FIX where both lists have at most 64 chunks
    "fixlds0": {"EK_KL_FIXLDS": "0"},                # the carved LDS layout
    "gbits": {"EK_KL_GBITS": "1"},                   # bitmaps off chip, 4096-position chunks
    "pipe": {"EK_KL_PIPE": "1"},                     # k_kl_swap_pipe
    "global": {"EK_KL_GLOBAL_STATE": "1"},           # k_kl_loop
    "noseg": {"EK_KL_NOSEG": "1"},                   # no inline rows: the CSR walk
    "nosegc": {"EK_KL_NOSEGC": "1"},                 # plain inline rows
    "gbits+nosegc": {"EK_KL_GBITS": "1", "EK_KL_NOSEGC": "1"},
    "pipe+nosegc": {"EK_KL_PIPE": "1", "EK_KL_NOSEGC": "1"},
}
ENV_NAMES = sorted({k for f in FORMS.values() for k in f})
LONG_FORMS = ("default", "gbits", "global")
PAIRS = [(f, n) for n in kc.cases() for f in FORMS if n not in kc.LONG or f in LONG_FORMS]


@pytest.fixture(scope="module")
def ctx(ek):
    c = ek.Context(0)
    yield c
    c.close()


def _bits(x):
    return np.float32(x).view(np.uint32)


def _set_form(monkeypatch, form):
    for k in ENV_NAMES:
        monkeypatch.delenv(k, raising=False)
    for k, v in FORMS[form].items():   # EK_KL_NOSEGC is read by kl_graph_setup, the rest by kl_run
        monkeypatch.setenv(k, v)


def _check(ctx, c, ref):
    log, res = ctx.kl_run(c.limit)
    swap_fields_equal(log, ref.log)
    assert res["iterations"] == ref.res["iterations"] and res["best_iter"] == ref.res["best_iter"]
    for k in ("initial_cut", "best_cut", "final_cut"):
        assert _bits(res[k]) == _bits(ref.res[k]), (k, res[k], ref.res[k])
    assert np.array_equal(ctx.kl_sides(0), ref.sides_init)
    assert np.array_equal(ctx.kl_sides(1), ref.sides_best)
    assert np.array_equal(ctx.kl_sides(2), ref.sides_final)
    if c.pins is not None:
        for k, s in (("net_cut_initial", ref.sides_init), ("net_cut_best", ref.sides_best),
                     ("net_cut_final", ref.sides_final)):
            assert res[k] == kc.net_cut(c.net_ptr, c.pins, s), k
    log2, res2 = ctx.kl_run(c.limit)   # the resident graph again
    swap_fields_equal(log2, ref.log)
    assert res2["best_iter"] == res["best_iter"]


@pytest.mark.parametrize("form,name", PAIRS)
def test_kl_shape(ek, ctx, monkeypatch, form, name):
    c, ref = kc.cases()[name], kc.reference(name)
    _set_form(monkeypatch, form)
    if c.pins is not None:
        G = ek.Hypergraph.from_pins(c.n, c.net_ptr, c.pins).kl_graph()
        assert np.array_equal(G.rowptr, c.rowptr) and np.array_equal(G.col, c.col)
        assert np.array_equal(np.asarray(G.val, np.float32).view(np.uint32), c.w.view(np.uint32))
        ctx.kl_graph_setup(G)
        ctx.kl_nets_setup(c.net_ptr, c.pins)
    else:
        ctx.kl_graph_setup(ek.CSR(c.rowptr, c.col, c.w))
        ctx.kl_nets_setup(np.zeros(1, np.int64), np.zeros(0, np.int32))   # no nets left over from another case
    ctx.kl_set_partition(c.order0, c.order1)
    _check(ctx, c, ref)


@pytest.mark.parametrize("form", ["default", "nosegc", "global"])
def test_kl_shape_from_bits(ek, ctx, monkeypatch, form):
    # kl_set_partition_bits on a direct CSR: the lists are the nodes of each side in ascending order
    c = kc.cases()["order-matters"]
    bits = np.zeros(c.n, np.uint8)
    bits[c.order1] = 1
    o0, o1 = np.flatnonzero(bits == 0), np.flatnonzero(bits == 1)
    ref = kc.reference_kl(c.rowptr, c.col, c.w, o0, o1, c.limit)
    _set_form(monkeypatch, form)
    ctx.kl_graph_setup(ek.CSR(c.rowptr, c.col, c.w))
    ctx.kl_nets_setup(np.zeros(1, np.int64), np.zeros(0, np.int32))
    ctx.kl_set_partition_bits(bits)
    _check(ctx, c, ref)
