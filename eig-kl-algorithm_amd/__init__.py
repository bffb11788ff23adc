"""eig-kl-algorithm_amd — Python mirror of the MI355X EIG+KL bipartitioner.

A thin ctypes layer over ``build/libeigkl_hip.so`` (C-ABI: include/eigkl.h).
It mirrors the reference's surface (yhinai/EIG-KL-Algorithm):

* ``cEIG(path)``, ``cKL(path, EIG=False)``, ``gKL(...)``, ``gKL2(...)`` run the
  drop-in tools in-process with the reference's argv/CWD semantics
  (cEIG.cpp:138-237, cKL.cpp:424-468, gKL.cu:672-713, gKL2.cu:989-1033);
* ``Hypergraph`` (read / generate / clique expansions), ``Context`` (SpMV seam,
  Lanczos Fiedler solver, KL swap loop) expose the hot path piecewise.

There is no CPU fallback: importing fails loudly when the HIP library has not
been built, and GPU calls raise ``EKError`` when no gfx950 device is usable.
The directory name is not a Python identifier; load it with
``importlib`` (see ``load()`` in tests/conftest.py or __graft_entry__.py).
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# EK_LIB_PATH: a design lab's A/B build of the same library (profiles/r03/scripts/ab_lab.sh)
LIB_PATH = os.environ.get("EK_LIB_PATH") or os.path.join(HERE, "build", "libeigkl_hip.so")
BIN_DIR = os.path.join(HERE, "build", "bin")

if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is not built: run `make -C {HERE}` "
                      "(the HIP path has no CPU fallback)")

_lib = ctypes.CDLL(LIB_PATH)
_P = ctypes.c_void_p
_I64 = ctypes.c_int64
_I32 = ctypes.c_int32

EK_OK, EK_EINVAL, EK_EIO, EK_EHIP, EK_ENOMEM, EK_ENOCONV, EK_ESTATE, EK_ECOMM = 0, -1, -2, -3, -4, -5, -6, -7

SWAP_DTYPE = np.dtype([("iter", "<u4"), ("node_left", "<u4"), ("node_right", "<u4"),
                       ("max_gain", "<f4"), ("min_gain", "<f4"), ("gain", "<f4"),
                       ("cut", "<f4"), ("pad", "<u4")])


class _AbiStruct(ctypes.Structure):
    """A mirror of an eigkl.h struct (layout ABI_VERSION): refused against a
    library that cannot state its ABI (an older EK_LIB_PATH lab build)."""

    def __init__(self, *a, **k):
        if not _ABI_CHECKED:
            raise RuntimeError(f"{type(self).__name__}: {_lib._name} has no ek_abi_version, its layout is unknown")
        super().__init__(*a, **k)


class LanczosOpts(_AbiStruct):
    _fields_ = [("ncv", _I32), ("maxit", _I32), ("tol", ctypes.c_double), ("deflate", _I32),
                ("time_spmv", _I32), ("reorth", _I32), ("check_every", _I32), ("basis32", _I32),
                ("alpha_last", _I32), ("keep_min", _I32), ("reorth_thresh", ctypes.c_double)]


class LanczosStats(_AbiStruct):
    _fields_ = [("restarts", _I32), ("matvecs", _I32), ("converged", _I32), ("residual", ctypes.c_double),
                ("total_ms", ctypes.c_double), ("spmv_ms", ctypes.c_double), ("spmv_timed", _I32),
                ("comm_ms", ctypes.c_double), ("allgathers", _I32), ("allreduces", _I32),
                ("update32_steps", _I32), ("update32_fallbacks", _I32), ("projected_steps", _I32),
                ("reprojected", _I32), ("ortho_max", ctypes.c_double)]


class KLResult(_AbiStruct):
    _fields_ = [("iterations", _I64), ("initial_cut", ctypes.c_float), ("best_cut", ctypes.c_float),
                ("final_cut", ctypes.c_float), ("best_iter", _I64), ("net_cut_initial", _I64),
                ("net_cut_best", _I64), ("net_cut_final", _I64), ("loop_ms", ctypes.c_double),
                ("total_ms", ctypes.c_double)]


class SolveOpts(_AbiStruct):
    _fields_ = [("eig", _I32), ("seed", ctypes.c_uint32), ("write_results", _I32), ("limit", _I32),
                ("out_dir", ctypes.c_char_p), ("sign_ref", ctypes.c_char_p), ("lanczos", LanczosOpts)]


_SOLVE_TIMES = ("t_read", "t_laplacian", "t_lanczos", "t_split", "t_kl_graph_wait", "t_kl_setup", "t_kl",
                "t_write", "t_total", "t_spmv_setup")


class SolveResult(_AbiStruct):
    _fields_ = ([("nets", _I64), ("nodes", _I64), ("pins", _I64), ("lambda_", ctypes.c_double),
                 ("median", ctypes.c_double), ("lanczos", LanczosStats), ("kl", KLResult)]
                + [(k, ctypes.c_double) for k in _SOLVE_TIMES])


KWAY_LEVELS = 8  # eigkl.h EK_KWAY_LEVELS


class KwayOpts(_AbiStruct):
    _fields_ = [("k", _I32), ("min_spectral", _I32), ("limit", _I32), ("write_results", _I32),
                ("out_dir", ctypes.c_char_p), ("lanczos", LanczosOpts)]


_KWAY_TIMES = ("t_induce", "t_lanczos", "t_kl", "t_metrics", "t_total")


class KwayResult(_AbiStruct):
    _fields_ = ([("k", _I32), ("bisections", _I32), ("fallback_splits", _I32), ("pad", _I32),
                 ("part_min", _I64), ("part_max", _I64), ("cut_nets", _I64), ("connectivity", _I64),
                 ("soed", _I64), ("matvecs", _I64), ("kl_swaps", _I64)]
                + [(k, ctypes.c_double) for k in _KWAY_TIMES] + [("t_level", ctypes.c_double * KWAY_LEVELS)])


class KwayRefineOpts(_AbiStruct):
    _fields_ = [("k", _I32), ("max_rounds", _I32), ("imbalance", ctypes.c_double)]


_REFINE_TIMES = ("t_setup", "t_rounds", "t_metrics")


class KwayRefineResult(_AbiStruct):
    _fields_ = ([("k", _I32), ("rounds", _I32)]
                + [(k, _I64) for k in ("moves", "gain_total", "max_part", "part_min", "part_max",
                                       "connectivity_before", "cut_nets", "connectivity", "soed")]
                + [(k, ctypes.c_double) for k in _REFINE_TIMES])


class KwayRefineWResult(_AbiStruct):
    _fields_ = ([("k", _I32), ("rounds", _I32)]
                + [(k, _I64) for k in ("moves", "gain_total", "total_weight", "bound_min", "bound_max", "part_w_min",
                                       "part_w_max", "parts_over_bound", "connectivity_w_before", "cut_nets",
                                       "connectivity", "connectivity_w", "soed")]
                + [(k, ctypes.c_double) for k in _REFINE_TIMES])


class KwayJetOpts(_AbiStruct):
    _fields_ = [("k", _I32), ("max_iters", _I32), ("patience", _I32), ("neg_num", _I32), ("neg_den", _I32),
                ("pad", _I32), ("imbalance", ctypes.c_double)]


class KwayJetResult(_AbiStruct):
    _fields_ = ([("k", _I32), ("iters", _I32), ("best_iter", _I32), ("pad", _I32)]
                + [(k, _I64) for k in ("moves", "total_weight", "bound_min", "bound_max", "connectivity_w_before",
                                       "cut_nets", "connectivity", "connectivity_w", "soed", "part_w_min",
                                       "part_w_max", "parts_over_bound")]
                + [(k, ctypes.c_double) for k in ("t_setup", "t_iters", "t_metrics")])


class KwayRebalanceOpts(_AbiStruct):
    _fields_ = [("k", _I32), ("max_rounds", _I32), ("imbalance", ctypes.c_double)]


class KwayRebalanceResult(_AbiStruct):
    _fields_ = ([("k", _I32), ("rounds", _I32)]
                + [(k, _I64) for k in ("moves", "total_weight", "bound_min", "bound_max", "parts_over_before",
                                       "parts_over_bound", "excess_before", "excess", "connectivity_w_before",
                                       "connectivity_w", "cut_nets", "connectivity", "soed", "part_w_min",
                                       "part_w_max")]
                + [(k, ctypes.c_double) for k in ("t_setup", "t_rounds", "t_metrics")])


class SweepOpts(_AbiStruct):
    _fields_ = [("objective", _I32), ("pad", _I32), ("imbalance", ctypes.c_double)]


_SWEEP_TIMES = ("t_sort", "t_profile", "t_select")


class SweepResult(_AbiStruct):
    _fields_ = ([(k, _I64) for k in ("n", "n0", "n1", "s_lo", "s_hi", "max_part", "cut", "cut_mid", "spanning_nets")]
                + [(k, ctypes.c_double) for k in _SWEEP_TIMES])


class SweepWResult(_AbiStruct):
    """eigkl.h ek_sweep_w_result (the weighted sweep cut)."""
    _fields_ = ([(k, _I64) for k in ("n", "n0", "n1", "s_lo", "s_hi", "feasible", "total_weight", "max_part", "w0", "w1",
                                     "cut", "cut_nets", "cut_half", "spanning_nets")]
                + [(k, ctypes.c_double) for k in _SWEEP_TIMES])


FM_CHUNK = 256  # ek_internal.hpp FM_CHUNK: node ids per chunk key of the FM pass
FM_LDS_CHUNKS = 2048  # ek_internal.hpp FM_LDS_CHUNKS: above this many chunks the keys live in global memory
FM_THREADS = 512  # ek_internal.hpp FM_THREADS: the FM pass's one workgroup

FM_MOVE_DTYPE = np.dtype([("node", "<i4"), ("gain", "<i4"), ("cut", "<i8")])  # eigkl.h ek_fm_move


class FmOpts(_AbiStruct):
    _fields_ = [("imbalance", ctypes.c_double), ("max_passes", _I32), ("stall", _I32)]


_FM_TIMES = ("t_setup", "t_passes", "t_metrics")


class FmResult(_AbiStruct):
    _fields_ = ([("n", _I64), ("max_part", _I64), ("passes", _I32), ("passes_run", _I32)]
                + [(k, _I64) for k in ("moves_tried", "moves_kept", "cut_before", "cut", "n0", "n1")]
                + [(k, ctypes.c_double) for k in _FM_TIMES])


class FmWResult(_AbiStruct):
    """eigkl.h ek_fm_w_result (the weighted FM refinement)."""
    _fields_ = ([("n", _I64), ("total_weight", _I64), ("max_part", _I64), ("passes", _I32), ("passes_run", _I32)]
                + [(k, _I64) for k in ("moves_tried", "moves_kept", "cut_before", "cut", "cut_nets_before", "cut_nets",
                                       "w0", "w1", "n0", "n1")]
                + [(k, ctypes.c_double) for k in _FM_TIMES])


MATCH_THREADS = 256  # ek_internal.hpp MATCH_THREADS: a workgroup of the matching's node kernels
MATCH_SHORT = 32  # ek_internal.hpp MATCH_SHORT: above this many entries a node is taken by its whole wave
ML_LEVELS = 32  # eigkl.h EK_ML_LEVELS


class MatchOpts(_AbiStruct):
    _fields_ = [("max_net", _I32), ("max_rounds", _I32), ("max_cluster", _I64)]


class MatchResult(_AbiStruct):
    _fields_ = [("n", _I64), ("n_coarse", _I64), ("pairs", _I64), ("rounds", _I32), ("pad", _I32),
                ("eligible_nets", _I64), ("t_setup", ctypes.c_double), ("t_rounds", ctypes.c_double)]


class ClusterResult(_AbiStruct):
    """eigkl.h ek_cluster_result (the multi-node clustering of the coarsening)."""
    _fields_ = [("n", _I64), ("n_coarse", _I64), ("joins", _I64), ("rounds", _I32), ("pad", _I32),
                ("eligible_nets", _I64), ("heaviest", _I64), ("t_setup", ctypes.c_double), ("t_rounds", ctypes.c_double)]


class MlOpts(_AbiStruct):
    _fields_ = [("imbalance", ctypes.c_double), ("coarse_nodes", _I32), ("max_levels", _I32), ("match", MatchOpts),
                ("fm", FmOpts), ("lanczos", LanczosOpts)]


_ML_LEVEL_FIELDS = ("nodes", "nets", "pins", "match_rounds", "match_pairs", "cut_before", "cut_after", "fm_moves")
_ML_INTS = ("sweep_feasible", "max_cluster", "total_weight", "max_part", "cut", "cut_nets", "w0", "w1", "n0", "n1")
_ML_TIMES = ("t_match", "t_contract", "t_lanczos", "t_sweep", "t_fm", "t_total")


class MlResult(_AbiStruct):
    """eigkl.h ek_ml_result (the multilevel bipartition)."""
    _fields_ = ([("levels", _I32), ("coarsest_fallback", _I32)]
                + [(k, _I64 * (ML_LEVELS + 1)) for k in _ML_LEVEL_FIELDS] + [(k, _I64) for k in _ML_INTS]
                + [(k, ctypes.c_double) for k in _ML_TIMES])


class SweepWBResult(_AbiStruct):
    """eigkl.h ek_sweep_wb_result (the weighted sweep cut under per-side bounds)."""
    _fields_ = ([(k, _I64) for k in ("n", "n0", "n1", "s_lo", "s_hi", "feasible", "total_weight", "bound0", "bound1",
                                     "w0", "w1", "cut", "cut_nets", "cut_half", "spanning_nets")]
                + [(k, ctypes.c_double) for k in _SWEEP_TIMES])


class FmWBResult(_AbiStruct):
    """eigkl.h ek_fm_wb_result (the weighted FM refinement under per-side bounds)."""
    _fields_ = ([("n", _I64), ("total_weight", _I64), ("bound0", _I64), ("bound1", _I64), ("passes", _I32),
                 ("passes_run", _I32)]
                + [(k, _I64) for k in ("moves_tried", "moves_kept", "cut_before", "cut", "cut_nets_before", "cut_nets",
                                       "w0", "w1", "n0", "n1")]
                + [(k, ctypes.c_double) for k in _FM_TIMES])


class KwayMlOpts(_AbiStruct):
    """eigkl.h ek_kway_ml_opts."""
    _fields_ = [("k", _I32), ("flags", _I32), ("imbalance", ctypes.c_double), ("write_results", _I32), ("pad", _I32),
                ("out_dir", ctypes.c_char_p), ("ml", MlOpts)]


_KWAY_ML_INTS = ("total_weight", "part_bound", "part_w_min", "part_w_max", "parts_over_bound", "empty_parts", "cut_nets",
                 "connectivity", "connectivity_w", "soed", "levels_total", "fm_moves")
_KWAY_ML_TIMES = ("t_induce", "t_ml", "t_metrics", "t_total", "t_match", "t_contract", "t_lanczos", "t_sweep", "t_fm")


class KwayMlResult(_AbiStruct):
    """eigkl.h ek_kway_ml_result."""
    _fields_ = ([("k", _I32), ("bisections", _I32), ("coarsest_fallbacks", _I32), ("infeasible_sweeps", _I32)]
                + [(k, _I64) for k in _KWAY_ML_INTS] + [(k, ctypes.c_double) for k in _KWAY_ML_TIMES]
                + [("t_level", ctypes.c_double * KWAY_LEVELS)])


class ContractOpts(_AbiStruct):
    """eigkl.h ek_contract_opts."""
    _fields_ = [("hash_bits", _I32), ("pad", _I32)]


KWAY_DIRECT_HOST_CONTRACT = 1  # eigkl.h EK_KWAY_DIRECT_HOST_CONTRACT
KWAY_DIRECT_WEIGHTED_LAPLACIAN = 2  # eigkl.h EK_KWAY_DIRECT_WEIGHTED_LAPLACIAN
COARSEN_MATCH = 0  # eigkl.h EK_COARSEN_MATCH
COARSEN_CLUSTER = 1  # eigkl.h EK_COARSEN_CLUSTER
_COARSENINGS = {"match": COARSEN_MATCH, "cluster": COARSEN_CLUSTER}


class KwayDirectOpts(_AbiStruct):
    """eigkl.h ek_kway_direct_opts."""
    _fields_ = [("k", _I32), ("flags", _I32), ("imbalance", ctypes.c_double), ("coarse_nodes", _I32),
                ("max_levels", _I32), ("match", MatchOpts), ("initial", KwayMlOpts), ("jet", KwayJetOpts),
                ("write_results", _I32), ("pad", _I32), ("out_dir", ctypes.c_char_p)]


_KWAY_DIRECT_LEVEL_FIELDS = ("nodes", "nets", "pins", "match_rounds", "match_pairs", "conn_w_before", "conn_w_after",
                             "jet_iters", "jet_moves")
_KWAY_DIRECT_INTS = ("total_weight", "part_bound", "max_cluster", "part_w_min", "part_w_max", "parts_over_bound",
                     "empty_parts", "cut_nets", "connectivity", "connectivity_w", "soed")
_KWAY_DIRECT_TIMES = ("t_match", "t_contract", "t_initial", "t_jet", "t_metrics", "t_total")


class KwayDirectResult(_AbiStruct):
    """eigkl.h ek_kway_direct_result."""
    _fields_ = ([("k", _I32), ("levels", _I32), ("initial_fallbacks", _I32), ("infeasible_sweeps", _I32)]
                + [(k, _I64 * (ML_LEVELS + 1)) for k in _KWAY_DIRECT_LEVEL_FIELDS]
                + [(k, _I64) for k in _KWAY_DIRECT_INTS] + [(k, ctypes.c_double) for k in _KWAY_DIRECT_TIMES])


_KWAY_DIRECT_RB_LEVEL_FIELDS = ("over_before", "excess_before", "rb_rounds", "rb_moves", "excess_after")


class KwayDirectRbResult(_AbiStruct):
    """eigkl.h ek_kway_direct_rb_result."""
    _fields_ = ([(k, _I64 * (ML_LEVELS + 1)) for k in _KWAY_DIRECT_RB_LEVEL_FIELDS]
                + [("t_rebalance", ctypes.c_double)])


ALLGATHER_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), _I64,
                                ctypes.POINTER(ctypes.c_double))
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), _I64)


def _sig(name, res, *args):
    try:
        fn = getattr(_lib, name)
    except AttributeError:
        if os.environ.get("EK_LIB_PATH"):  # (a lab's older A/B build: the entry is simply absent)
            return None
        raise
    fn.restype = res
    fn.argtypes = list(args)
    return fn


_sig("ek_last_error", ctypes.c_char_p)
_sig("ek_version", ctypes.c_char_p)
ABI_VERSION = 4  # eigkl.h EIGKL_ABI_VERSION: the ctypes struct mirrors below follow that layout
if _sig("ek_abi_version", ctypes.c_int) is not None:
    if _lib.ek_abi_version() != ABI_VERSION:
        raise ImportError(f"libeigkl_hip ABI {_lib.ek_abi_version()} != the {ABI_VERSION} these bindings mirror: rebuild")
    _ABI_CHECKED = True
else:
    # an EK_LIB_PATH lab build older than the ABI query: its struct layouts are
    # unknown, so every entry that takes one of the mirrors below refuses
    import warnings
    warnings.warn(f"{_lib._name} has no ek_abi_version: calls passing ABI-{ABI_VERSION} structs are refused")
    _ABI_CHECKED = False
_sig("ek_hgr_read", ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_P))
_sig("ek_hgr_generate", ctypes.c_int, ctypes.c_double, ctypes.c_uint64, ctypes.POINTER(_P))
_sig("ek_hgr_from_pins", ctypes.c_int, _I64, _I64, _P, _P, ctypes.POINTER(_P))
_sig("ek_hgr_write", ctypes.c_int, _P, ctypes.c_char_p)
_sig("ek_hgr_dims", ctypes.c_int, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64))
_sig("ek_hgr_copy_pins", ctypes.c_int, _P, _P, _P)
_sig("ek_hgr_free", None, _P)
_sig("ek_laplacian_build", ctypes.c_int, _P, ctypes.POINTER(_P))
_sig("ek_kl_graph_build", ctypes.c_int, _P, ctypes.POINTER(_P))
_sig("ek_laplacian_build_rows", ctypes.c_int, _P, _I64, _I64, ctypes.POINTER(_P))
_sig("ek_laplacian_build_w", ctypes.c_int, _P, ctypes.POINTER(_P))
_sig("ek_laplacian_build_rows_w", ctypes.c_int, _P, _I64, _I64, ctypes.POINTER(_P))
_sig("ek_synchronize", ctypes.c_int, _P)
_sig("ek_csr_dims", ctypes.c_int, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I32))
_sig("ek_csr_copy", ctypes.c_int, _P, _P, _P, _P, _P)
_sig("ek_csr_free", None, _P)
_sig("ek_shard_rows", ctypes.c_int, _I64, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_I64),
     ctypes.POINTER(_I64), ctypes.POINTER(_I64))
_sig("ek_shard_map", ctypes.c_int, _I64, _I64, _P, _P, ctypes.c_int, _P)
_sig("ek_device_count", ctypes.c_int, ctypes.POINTER(ctypes.c_int))
_sig("ek_init", ctypes.c_int, ctypes.c_int, ctypes.POINTER(_P))
_sig("ek_destroy", None, _P)
_sig("ek_get_stream", ctypes.c_int, _P, ctypes.POINTER(_P))
_sig("ek_comm_unique_id", ctypes.c_int, _P)
_sig("ek_comm_init", ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, _P)
_sig("ek_comm_init_host", ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ALLGATHER_FN, ALLREDUCE_FN, _P)
_sig("ek_hgr_largest_component", ctypes.c_int, _P, ctypes.POINTER(_P), _P)
_sig("ek_random_split", ctypes.c_int, _I64, ctypes.c_uint32, _P, _P)
_sig("ek_solve_default_opts", None, ctypes.POINTER(SolveOpts))
_sig("ek_solve_file", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(SolveOpts), _P, _I64,
     ctypes.POINTER(SolveResult))
_sig("ek_spmv_setup", ctypes.c_int, _P, _I64, _I64, _I64, _P, _P, _P)
_sig("ek_spmv", ctypes.c_int, _P, _P, _P, _P)
_sig("ek_spmv_setup_pins", ctypes.c_int, _P, _I64, _I64, _P, _P, ctypes.POINTER(ctypes.c_int32))
_sig("ek_spmv_setup_pins_w", ctypes.c_int, _P, _I64, _I64, _P, _P, _P, ctypes.POINTER(ctypes.c_int32))
_sig("ek_spmv_host", ctypes.c_int, _P, _P, _P)
_sig("ek_spmv_bytes", _I64, _P)
_sig("ek_spmv_dims", ctypes.c_int, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64))
_sig("ek_spmv_format", ctypes.c_int, _P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_I64))
_sig("ek_spmv_exchange", ctypes.c_int, _P, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(_I64), ctypes.POINTER(_I64))
_sig("ek_comm_stats", ctypes.c_int, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64), ctypes.POINTER(_I64),
     ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(_I64))
_sig("ek_spmv_gather_bench", ctypes.c_int, _P, ctypes.c_int, ctypes.POINTER(ctypes.c_double))
_sig("ek_spmv_bench", ctypes.c_int, _P, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double))
_sig("ek_lanczos_default_opts", None, ctypes.POINTER(LanczosOpts))
_sig("ek_lanczos_fiedler", ctypes.c_int, _P, ctypes.POINTER(LanczosOpts), ctypes.POINTER(ctypes.c_double), _P,
     ctypes.POINTER(LanczosStats))
_sig("ek_median_split", ctypes.c_int, _I64, _P, ctypes.POINTER(ctypes.c_double), _P)
_sig("ek_align_sign", ctypes.c_int, _I64, _P, _P)
_sig("ek_eig_write", ctypes.c_int, ctypes.c_char_p, _I64, ctypes.c_double, ctypes.c_double, _P, _P)
_sig("ek_eig_read", ctypes.c_int, ctypes.c_char_p, _I64, ctypes.POINTER(ctypes.c_double),
     ctypes.POINTER(ctypes.c_double), _P, _P, _P, ctypes.POINTER(_I64), _P, ctypes.POINTER(_I64))
_sig("ek_kl_graph_setup", ctypes.c_int, _P, _I64, _P, _P, _P)
_sig("ek_kl_nets_setup", ctypes.c_int, _P, _I64, _P, _P)
_sig("ek_kl_set_partition", ctypes.c_int, _P, _P, _I64, _P, _I64)
_sig("ek_kl_set_partition_bits", ctypes.c_int, _P, _I64, _P)
_sig("ek_kl_set_partition_fiedler", ctypes.c_int, _P, _P, _P, _P)
_sig("ek_fiedler_set", ctypes.c_int, _P, _I64, _P)
_sig("ek_kl_partition_copy", ctypes.c_int, _P, _P, _P, _P, _P, ctypes.POINTER(_I64), ctypes.POINTER(_I64))
_sig("ek_kl_run", ctypes.c_int, _P, _I32, _P, _I64, ctypes.POINTER(KLResult))
_sig("ek_kl_sides", ctypes.c_int, _P, _I32, _P)
_sig("ek_cli_main", ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_char_p))
_sig("ek_kway_plan", ctypes.c_int, _I64, _I32, _P)
_sig("ek_rank_split", ctypes.c_int, _I64, _P, _I64, _P)
_sig("ek_hgr_induce", ctypes.c_int, _P, _P, ctypes.POINTER(_P), _P)
_sig("ek_kway_metrics_host", ctypes.c_int, _I64, _P, _P, _P, _I32, _P)
_sig("ek_rank_split_device", ctypes.c_int, _P, _I64, _P, _I64, _P)
_sig("ek_kl_set_partition_fiedler_rank", ctypes.c_int, _P, _I64, ctypes.POINTER(_I64), ctypes.POINTER(_I64))
_sig("ek_kway_metrics", ctypes.c_int, _P, _I64, _P, _P, _P, _I32, _P)
_sig("ek_kway_default_opts", None, ctypes.POINTER(KwayOpts))
_sig("ek_partition_kway", ctypes.c_int, _P, _P, ctypes.POINTER(KwayOpts), _P, ctypes.POINTER(KwayResult))
_sig("ek_partition_kway_file", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(KwayOpts), _P,
     ctypes.POINTER(KwayResult))
_sig("ek_kway_refine_default_opts", None, ctypes.POINTER(KwayRefineOpts))
_sig("ek_kway_refine_host", ctypes.c_int, _P, ctypes.POINTER(KwayRefineOpts), _P, _P, _I64,
     ctypes.POINTER(KwayRefineResult))
_sig("ek_kway_refine", ctypes.c_int, _P, _P, ctypes.POINTER(KwayRefineOpts), _P, _P, _I64,
     ctypes.POINTER(KwayRefineResult))
_sig("ek_kway_refine_w_host", ctypes.c_int, _P, ctypes.POINTER(KwayRefineOpts), _P, _P, _P, _I64,
     ctypes.POINTER(KwayRefineWResult))
_sig("ek_kway_refine_w", ctypes.c_int, _P, _P, ctypes.POINTER(KwayRefineOpts), _P, _P, _P, _I64,
     ctypes.POINTER(KwayRefineWResult))
_sig("ek_kway_jet_default_opts", None, ctypes.POINTER(KwayJetOpts))
_sig("ek_kway_jet_host", ctypes.c_int, _P, ctypes.POINTER(KwayJetOpts), _P, _P, _P, _I64,
     ctypes.POINTER(KwayJetResult))
_sig("ek_kway_jet", ctypes.c_int, _P, _P, ctypes.POINTER(KwayJetOpts), _P, _P, _P, _I64,
     ctypes.POINTER(KwayJetResult))
_sig("ek_kway_rebalance_default_opts", None, ctypes.POINTER(KwayRebalanceOpts))
_sig("ek_kway_rebalance_host", ctypes.c_int, _P, ctypes.POINTER(KwayRebalanceOpts), _P, _P, _P, _I64,
     ctypes.POINTER(KwayRebalanceResult))
_sig("ek_kway_rebalance", ctypes.c_int, _P, _P, ctypes.POINTER(KwayRebalanceOpts), _P, _P, _P, _I64,
     ctypes.POINTER(KwayRebalanceResult))
_sig("ek_sweep_default_opts", None, ctypes.POINTER(SweepOpts))
_sig("ek_sweep_cut_host", ctypes.c_int, _P, _P, ctypes.POINTER(SweepOpts), _P, _P, ctypes.POINTER(SweepResult))
_sig("ek_sweep_cut", ctypes.c_int, _P, _P, _P, ctypes.POINTER(SweepOpts), _P, _P, ctypes.POINTER(SweepResult))
_sig("ek_kl_set_partition_fiedler_sweep", ctypes.c_int, _P, _P, ctypes.POINTER(SweepOpts),
     ctypes.POINTER(SweepResult))
_sig("ek_sweep_cut_w_host", ctypes.c_int, _P, _P, ctypes.POINTER(SweepOpts), _P, _P, _P, ctypes.POINTER(SweepWResult))
_sig("ek_sweep_cut_w", ctypes.c_int, _P, _P, _P, ctypes.POINTER(SweepOpts), _P, _P, _P, ctypes.POINTER(SweepWResult))
_sig("ek_kl_set_partition_fiedler_sweep_w", ctypes.c_int, _P, _P, ctypes.POINTER(SweepOpts),
     ctypes.POINTER(SweepWResult))
_sig("ek_fm_default_opts", None, ctypes.POINTER(FmOpts))
_sig("ek_fm_refine_host", ctypes.c_int, _P, ctypes.POINTER(FmOpts), _P, _P, _I64, _P, _I64, ctypes.POINTER(FmResult))
_sig("ek_fm_refine", ctypes.c_int, _P, _P, ctypes.POINTER(FmOpts), _P, _P, _I64, _P, _I64, ctypes.POINTER(FmResult))
_sig("ek_hgr_set_weights", ctypes.c_int, _P, _P, _P)
_sig("ek_hgr_weights", ctypes.c_int, _P, ctypes.POINTER(_I32), ctypes.POINTER(_I32))
_sig("ek_hgr_copy_weights", ctypes.c_int, _P, _P, _P)
_sig("ek_hgr_read_weighted", ctypes.c_int, ctypes.c_char_p, ctypes.POINTER(_P))
_sig("ek_bipart_metrics_host", ctypes.c_int, _P, _P, _P)
_sig("ek_fm_refine_w_host", ctypes.c_int, _P, ctypes.POINTER(FmOpts), _P, _P, _I64, _P, _I64,
     ctypes.POINTER(FmWResult))
_sig("ek_fm_refine_w", ctypes.c_int, _P, _P, ctypes.POINTER(FmOpts), _P, _P, _I64, _P, _I64,
     ctypes.POINTER(FmWResult))
_sig("ek_match_default_opts", None, ctypes.POINTER(MatchOpts))
_sig("ek_match_host", ctypes.c_int, _P, ctypes.POINTER(MatchOpts), _P, _P, _P, _I64, ctypes.POINTER(MatchResult))
_sig("ek_match", ctypes.c_int, _P, _P, ctypes.POINTER(MatchOpts), _P, _P, _P, _I64, ctypes.POINTER(MatchResult))
_sig("ek_cluster_host", ctypes.c_int, _P, ctypes.POINTER(MatchOpts), _P, _P, _P, _I64, ctypes.POINTER(ClusterResult))
_sig("ek_cluster", ctypes.c_int, _P, _P, ctypes.POINTER(MatchOpts), _P, _P, _P, _I64, ctypes.POINTER(ClusterResult))
_sig("ek_hgr_contract", ctypes.c_int, _P, _P, _I64, ctypes.POINTER(_P))
_sig("ek_ml_default_opts", None, ctypes.POINTER(MlOpts))
_sig("ek_multilevel_bipartition", ctypes.c_int, _P, _P, ctypes.POINTER(MlOpts), _P, ctypes.POINTER(MlResult))
_sig("ek_multilevel_bipartition_file", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(MlOpts), ctypes.c_char_p, _P,
     ctypes.POINTER(MlResult))
_sig("ek_multilevel_bipartition_ex", ctypes.c_int, _P, _P, ctypes.POINTER(MlOpts), _I32, _P, ctypes.POINTER(MlResult))
_sig("ek_multilevel_bipartition_file_ex", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(MlOpts), ctypes.c_char_p,
     _I32, _P, ctypes.POINTER(MlResult))
ML_WEIGHTED_LAPLACIAN = 1  # eigkl.h EK_ML_WEIGHTED_LAPLACIAN
_sig("ek_sweep_cut_wb_host", ctypes.c_int, _P, _P, ctypes.POINTER(SweepOpts), _P, _P, _P, _P,
     ctypes.POINTER(SweepWBResult))
_sig("ek_sweep_cut_wb", ctypes.c_int, _P, _P, _P, ctypes.POINTER(SweepOpts), _P, _P, _P, _P,
     ctypes.POINTER(SweepWBResult))
_sig("ek_fm_refine_wb_host", ctypes.c_int, _P, ctypes.POINTER(FmOpts), _P, _P, _P, _I64, _P, _I64,
     ctypes.POINTER(FmWBResult))
_sig("ek_fm_refine_wb", ctypes.c_int, _P, _P, ctypes.POINTER(FmOpts), _P, _P, _P, _I64, _P, _I64,
     ctypes.POINTER(FmWBResult))
_sig("ek_multilevel_bipartition_b", ctypes.c_int, _P, _P, ctypes.POINTER(MlOpts), _I32, _P, _P, ctypes.POINTER(MlResult))
_sig("ek_kway_bisect_bounds", ctypes.c_int, _I64, _I32, _I64, ctypes.c_double, _P)
_sig("ek_kway_metrics_w_host", ctypes.c_int, _P, _P, _I32, _P)
_sig("ek_kway_metrics_w", ctypes.c_int, _P, _P, _P, _I32, _P)
_sig("ek_kway_ml_default_opts", None, ctypes.POINTER(KwayMlOpts))
_sig("ek_partition_kway_ml", ctypes.c_int, _P, _P, ctypes.POINTER(KwayMlOpts), _P, ctypes.POINTER(KwayMlResult))
_sig("ek_partition_kway_ml_file", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(KwayMlOpts), _P,
     ctypes.POINTER(KwayMlResult))
_sig("ek_contract_default_opts", None, ctypes.POINTER(ContractOpts))
_sig("ek_hgr_contract_device", ctypes.c_int, _P, _P, _P, _I64, ctypes.POINTER(ContractOpts), ctypes.POINTER(_P))
_sig("ek_kway_direct_default_opts", None, ctypes.POINTER(KwayDirectOpts))
_sig("ek_partition_kway_direct", ctypes.c_int, _P, _P, ctypes.POINTER(KwayDirectOpts), _P,
     ctypes.POINTER(KwayDirectResult))
_sig("ek_partition_kway_direct_file", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(KwayDirectOpts), _P,
     ctypes.POINTER(KwayDirectResult))
_sig("ek_partition_kway_direct_ex", ctypes.c_int, _P, _P, ctypes.POINTER(KwayDirectOpts), _I32, _P,
     ctypes.POINTER(KwayDirectResult))
_sig("ek_partition_kway_direct_file_ex", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(KwayDirectOpts), _I32, _P,
     ctypes.POINTER(KwayDirectResult))
_sig("ek_partition_kway_direct_rb", ctypes.c_int, _P, _P, ctypes.POINTER(KwayDirectOpts), _I32, _P,
     ctypes.POINTER(KwayDirectResult), ctypes.POINTER(KwayDirectRbResult))
_sig("ek_partition_kway_direct_rb_file", ctypes.c_int, _P, ctypes.c_char_p, ctypes.POINTER(KwayDirectOpts), _I32, _P,
     ctypes.POINTER(KwayDirectResult), ctypes.POINTER(KwayDirectRbResult))

lib = _lib


class EKError(RuntimeError):
    def __init__(self, code, what):
        super().__init__(f"{what}: {_lib.ek_last_error().decode(errors='replace')} (status {code})")
        self.code = code


def _chk(rc, what):
    if rc != EK_OK:
        raise EKError(rc, what)


def _p(a):
    return a.ctypes.data_as(_P) if a is not None else None


def version():
    return _lib.ek_version().decode()


# ---------------------------------------------------------------------------
# host side
class CSR:
    def __init__(self, rowptr, col, val, nfwd=None):
        self.rowptr, self.col, self.val, self.nfwd = rowptr, col, val, nfwd

    @property
    def nrows(self):
        return len(self.rowptr) - 1

    @property
    def nnz(self):
        return len(self.col)


def _take_csr(handle):
    nr, nnz, vb = _I64(), _I64(), _I32()
    _lib.ek_csr_dims(handle, ctypes.byref(nr), ctypes.byref(nnz), ctypes.byref(vb))
    rowptr = np.empty(nr.value + 1, np.int32)
    col = np.empty(nnz.value, np.int32)
    val = np.empty(nnz.value, np.float64 if vb.value == 8 else np.float32)
    nfwd = np.empty(nr.value, np.int32) if vb.value == 4 else None
    _lib.ek_csr_copy(handle, _p(rowptr), _p(col), _p(val), _p(nfwd))
    _lib.ek_csr_free(handle)
    return CSR(rowptr, col, val, nfwd)


class Hypergraph:
    """A .hgr circuit (cKL.cpp:84-116 / cEIG.cpp:177-182 readers)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def read(cls, path):
        h = _P()
        _chk(_lib.ek_hgr_read(os.fsencode(path), ctypes.byref(h)), f"read {path}")
        return cls(h)

    @classmethod
    def generate(cls, multiplier=1.0, seed=1):
        """Seeded ISPD98-shaped synthetic circuit (circuit_generator.py:41-59)."""
        h = _P()
        _chk(_lib.ek_hgr_generate(float(multiplier), int(seed), ctypes.byref(h)), "generate")
        return cls(h)

    @classmethod
    def from_pins(cls, nodes, net_ptr, pins):
        net_ptr = np.ascontiguousarray(net_ptr, np.int64)
        pins = np.ascontiguousarray(pins, np.int32)
        h = _P()
        _chk(_lib.ek_hgr_from_pins(len(net_ptr) - 1, int(nodes), _p(net_ptr), _p(pins), ctypes.byref(h)),
             "from_pins")
        return cls(h)

    @classmethod
    def read_weighted(cls, path):
        """The hMETIS reading of a .hgr file (ek_hgr_read_weighted): header `nets nodes [fmt]`, fmt 1 / 11 with a
        weight at the head of every net line, fmt 10 / 11 with one node weight line per node, `%` comments."""
        h = _P()
        _chk(_lib.ek_hgr_read_weighted(os.fsencode(path), ctypes.byref(h)), f"read_weighted {path}")
        return cls(h)

    def set_weights(self, node_w=None, net_w=None):
        """Node weights (>= 0, one per node) and net weights (>= 1, one per net); None clears that array, which
        then stands for all ones (ek_hgr_set_weights).  Only the weighted FM refinement, the weighted sweep cut
        and bipart_metrics_host read them."""
        nets, nodes, _ = self.dims()
        node_w = None if node_w is None else np.ascontiguousarray(node_w, np.int32)
        net_w = None if net_w is None else np.ascontiguousarray(net_w, np.int32)
        if node_w is not None and len(node_w) != nodes:
            raise ValueError(f"node_w has {len(node_w)} entries for {nodes} nodes")
        if net_w is not None and len(net_w) != nets:
            raise ValueError(f"net_w has {len(net_w)} entries for {nets} nets")
        _chk(_lib.ek_hgr_set_weights(self._h, _p(node_w), _p(net_w)), "set_weights")

    def weights(self):
        """(node_w, net_w): each an int32 array, or None for an array the hypergraph does not carry."""
        nets, nodes, _ = self.dims()
        hn, he = _I32(), _I32()
        _chk(_lib.ek_hgr_weights(self._h, ctypes.byref(hn), ctypes.byref(he)), "weights")
        node_w = np.empty(nodes, np.int32) if hn.value else None
        net_w = np.empty(nets, np.int32) if he.value else None
        _chk(_lib.ek_hgr_copy_weights(self._h, _p(node_w), _p(net_w)), "weights")
        return node_w, net_w

    def __del__(self):
        if getattr(self, "_h", None):
            _lib.ek_hgr_free(self._h)
            self._h = None

    def dims(self):
        a, b, c = _I64(), _I64(), _I64()
        _lib.ek_hgr_dims(self._h, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
        return a.value, b.value, c.value

    @property
    def nets(self):
        return self.dims()[0]

    @property
    def nodes(self):
        return self.dims()[1]

    def pins(self):
        nets, _, npins = self.dims()
        net_ptr = np.empty(nets + 1, np.int64)
        pins = np.empty(npins, np.int32)
        _lib.ek_hgr_copy_pins(self._h, _p(net_ptr), _p(pins))
        return net_ptr, pins

    def write(self, path):
        _chk(_lib.ek_hgr_write(self._h, os.fsencode(path)), f"write {path}")

    def largest_component(self):
        """(Hypergraph of the largest connected component, node map old -> new or -1)."""
        c = _P()
        m = np.empty(self.nodes, np.int32)
        _chk(_lib.ek_hgr_largest_component(self._h, ctypes.byref(c), _p(m)), "largest_component")
        return Hypergraph(c), m

    def induce(self, keep):
        """(sub-hypergraph on the nodes with keep != 0, node map old -> new or -1): nets restricted to their
        kept pins, those left with fewer than 2 dropped (ek_hgr_induce)."""
        keep = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
        if len(keep) != self.nodes:
            raise ValueError(f"keep has {len(keep)} entries for {self.nodes} nodes")
        c = _P()
        m = np.empty(self.nodes, np.int32)
        _chk(_lib.ek_hgr_induce(self._h, _p(keep), ctypes.byref(c), _p(m)), "induce")
        return Hypergraph(c), m

    def contract(self, cluster, n_coarse=None):
        """The contraction along cluster, a map of the nodes onto [0, n_coarse) that hits every value
        (ek_hgr_contract): cluster weights summed, nets mapped and made distinct, those left with fewer than 2 pins
        dropped, nets of one pin set merged with their weights summed.  n_coarse: max(cluster) + 1 by default."""
        cluster = np.ascontiguousarray(cluster, np.int32)
        if len(cluster) != self.nodes:
            raise ValueError(f"cluster has {len(cluster)} entries for {self.nodes} nodes")
        if n_coarse is None:
            n_coarse = int(cluster.max()) + 1 if len(cluster) else 0
        c = _P()
        _chk(_lib.ek_hgr_contract(self._h, _p(cluster), int(n_coarse), ctypes.byref(c)), "contract")
        return Hypergraph(c)

    def laplacian(self, weighted=False):
        """fp64 clique Laplacian (cEIG.cpp:86-133).  weighted: -(2 c(e) / |e|) per pin pair, c(e) the net weights
        (ek_laplacian_build_w); without net weights the same arrays."""
        c = _P()
        build = _lib.ek_laplacian_build_w if weighted else _lib.ek_laplacian_build
        _chk(build(self._h, ctypes.byref(c)), "laplacian")
        return _take_csr(c)

    def laplacian_rows(self, row0, row1, weighted=False):
        """Rows [row0, row1) of the Laplacian (global columns, rowptr from 0): one rank's shard.  weighted: as
        laplacian (ek_laplacian_build_rows_w)."""
        c = _P()
        build = _lib.ek_laplacian_build_rows_w if weighted else _lib.ek_laplacian_build_rows
        _chk(build(self._h, int(row0), int(row1 - row0), ctypes.byref(c)), "laplacian_rows")
        return _take_csr(c)

    def kl_graph(self):
        """fp32 KL adjacency in cKL summation order (cKL.cpp:84-149, 225-251)."""
        c = _P()
        _chk(_lib.ek_kl_graph_build(self._h, ctypes.byref(c)), "kl_graph")
        return _take_csr(c)


def shard_rows(n, nranks, rank):
    a, b, c = _I64(), _I64(), _I64()
    _chk(_lib.ek_shard_rows(int(n), int(nranks), int(rank), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
         "shard_rows")
    return a.value, b.value, c.value


def shard_map(hgr, nranks):
    """nnz-balanced row offsets (nranks + 1) of the sharded Lanczos (ek_shard_map): rank r owns
    [off[r], off[r+1]); the map ek_spmv_setup_pins uses."""
    net_ptr, pins = hgr.pins()
    off = np.empty(int(nranks) + 1, np.int64)
    _chk(_lib.ek_shard_map(int(hgr.nodes), len(net_ptr) - 1, _p(net_ptr), _p(pins), int(nranks), _p(off)),
         "shard_map")
    return off


def median_split(v):
    """cEIG.cpp:55-65, 218: median and bits = (median > v)."""
    v = np.ascontiguousarray(v, np.float64)
    med = ctypes.c_double()
    bits = np.empty(len(v), np.uint8)
    _chk(_lib.ek_median_split(len(v), _p(v), ctypes.byref(med), _p(bits)), "median_split")
    return med.value, bits


def kway_plan(n, k):
    """Part sizes of the k-way recursion (ek_kway_plan): each floor(n/k) or ceil(n/k)."""
    sizes = np.zeros(max(int(k), 1), np.int64)
    _chk(_lib.ek_kway_plan(int(n), int(k), _p(sizes)), "kway_plan")
    return sizes


def rank_split(v, n1):
    """bits = 1 for the n1 nodes smallest in (radix order of v, node id) (ek_rank_split)."""
    v = np.ascontiguousarray(v, np.float64)
    bits = np.empty(len(v), np.uint8)
    _chk(_lib.ek_rank_split(len(v), _p(v), int(n1), _p(bits)), "rank_split")
    return bits


def kway_metrics_host(net_ptr, pins, part, k):
    """(cut nets, connectivity, SOED) of a part vector, on the host (ek_kway_metrics_host)."""
    net_ptr = np.ascontiguousarray(net_ptr, np.int64)
    pins = np.ascontiguousarray(pins, np.int32)
    part = np.ascontiguousarray(part, np.int32)
    if len(pins) and int(pins.max()) >= len(part):
        raise ValueError("part is shorter than the pins' node range")
    out = np.zeros(3, np.int64)
    _chk(_lib.ek_kway_metrics_host(len(net_ptr) - 1, _p(net_ptr), _p(pins), _p(part), int(k), _p(out)),
         "kway_metrics_host")
    return tuple(int(x) for x in out)


def _kway_opts(k, min_spectral, limit, write_results, out_dir, lanczos):
    o = KwayOpts()
    _lib.ek_kway_default_opts(ctypes.byref(o))
    o.k, o.min_spectral, o.limit, o.write_results = int(k), int(min_spectral), int(limit), 1 if write_results else 0
    o.out_dir = os.fsencode(out_dir) if out_dir else None
    for name, val in (lanczos or {}).items():
        setattr(o.lanczos, name, val)
    return o


def _kway_result(r):
    out = {k: getattr(r, k) for k, _ in KwayResult._fields_ if k not in ("pad", "t_level")}
    out["t_level"] = list(r.t_level)
    return out


def _kway_refine(call, what, hgr, part, k, imbalance, max_rounds):
    """(refined part, result dict, round log): the log has one row per round that
    moved, (candidates, independent candidates, accepted moves, gain)."""
    start = np.ascontiguousarray(part, np.int32)
    if len(start) != hgr.nodes:
        raise ValueError(f"part has {len(start)} entries for {hgr.nodes} nodes")
    o = KwayRefineOpts()
    _lib.ek_kway_refine_default_opts(ctypes.byref(o))
    o.k, o.max_rounds, o.imbalance = int(k), int(max_rounds), float(imbalance)
    cap = int(max_rounds) if max_rounds > 0 else 1024
    while True:
        out = start.copy()
        log = np.zeros((cap, 4), np.int64)
        r = KwayRefineResult()
        _chk(call(ctypes.byref(o), _p(out), _p(log), cap, ctypes.byref(r)), what)
        if r.rounds <= cap:  # (else: deterministic, so the same run again with room for its log)
            break
        cap = r.rounds
    return out, {name: getattr(r, name) for name, _ in KwayRefineResult._fields_}, log[:r.rounds].copy()


def kway_refine_host(hgr, part, k, imbalance=0.03, max_rounds=0):
    """k-way connectivity refinement under L_max = floor((1 + imbalance) ceil(n / k)), on the host
    (ek_kway_refine_host, the device path's checker).  Returns (part, result dict, round log)."""
    return _kway_refine(lambda *a: _lib.ek_kway_refine_host(hgr._h, *a), "kway_refine_host", hgr, part, k,
                        imbalance, max_rounds)


def _kway_refine_w(call, what, hgr, part, k, imbalance, max_rounds, bounds):
    """_kway_refine for the weighted entries: bounds is None (the uniform bound at `imbalance`) or k int64 values."""
    start = np.ascontiguousarray(part, np.int32)
    if len(start) != hgr.nodes:
        raise ValueError(f"part has {len(start)} entries for {hgr.nodes} nodes")
    if bounds is not None:
        bounds = np.ascontiguousarray(bounds, np.int64)
        if len(bounds) != int(k):
            raise ValueError(f"{len(bounds)} bounds for {k} parts")
    o = KwayRefineOpts()
    _lib.ek_kway_refine_default_opts(ctypes.byref(o))
    o.k, o.max_rounds, o.imbalance = int(k), int(max_rounds), float(imbalance)
    cap = int(max_rounds) if max_rounds > 0 else 1024
    while True:
        out = start.copy()
        log = np.zeros((cap, 4), np.int64)
        r = KwayRefineWResult()
        _chk(call(ctypes.byref(o), _p(bounds), _p(out), _p(log), cap, ctypes.byref(r)), what)
        if r.rounds <= cap:  # (else: deterministic, so the same run again with room for its log)
            break
        cap = r.rounds
    return out, {name: getattr(r, name) for name, _ in KwayRefineWResult._fields_}, log[:r.rounds].copy()


def kway_refine_w_host(hgr, part, k, imbalance=0.03, max_rounds=0, bounds=None):
    """Weighted k-way connectivity refinement under per-part weight bounds, on the host (ek_kway_refine_w_host, the
    device path's checker): hgr's node weights under bounds[p], or under floor((1 + imbalance) ceil(W / k)) when
    bounds is None, its net weights in the connectivity.  Returns (part, result dict, round log)."""
    return _kway_refine_w(lambda *a: _lib.ek_kway_refine_w_host(hgr._h, *a), "kway_refine_w_host", hgr, part, k,
                          imbalance, max_rounds, bounds)


def _kway_jet(call, what, hgr, part, k, imbalance, bounds, max_iters, patience, neg):
    """_kway_refine_w for the Jet entries: neg is the negative-gain filter (neg_num, neg_den)."""
    start = np.ascontiguousarray(part, np.int32)
    if len(start) != hgr.nodes:
        raise ValueError(f"part has {len(start)} entries for {hgr.nodes} nodes")
    if bounds is not None:
        bounds = np.ascontiguousarray(bounds, np.int64)
        if len(bounds) != int(k):
            raise ValueError(f"{len(bounds)} bounds for {k} parts")
    o = KwayJetOpts()
    _lib.ek_kway_jet_default_opts(ctypes.byref(o))
    o.k, o.max_iters, o.patience, o.imbalance = int(k), int(max_iters), int(patience), float(imbalance)
    o.neg_num, o.neg_den = int(neg[0]), int(neg[1])
    cap = int(max_iters) if max_iters > 0 else 256
    while True:
        out = start.copy()
        log = np.zeros((cap, 4), np.int64)
        r = KwayJetResult()
        _chk(call(ctypes.byref(o), _p(bounds), _p(out), _p(log), cap, ctypes.byref(r)), what)
        if r.iters <= cap:  # (else: deterministic, so the same run again with room for its log)
            break
        cap = r.iters
    res = {name: getattr(r, name) for name, _ in KwayJetResult._fields_ if name != "pad"}
    return out, res, log[:r.iters].copy()


def kway_jet_host(hgr, part, k, eps=0.03, bounds=None, max_iters=0, patience=12, neg=(1, 4)):
    """Parallel weighted k-way refinement that can leave a local minimum (the Jet rule on the weighted connectivity),
    on the host (ek_kway_jet_host, the device path's checker): hgr's node weights under bounds[p], or under
    floor((1 + eps) ceil(W / k)) when bounds is None.  Returns (part, result dict, iteration log); a log row is
    (candidates, passing candidates, accepted moves, the weighted connectivity after the iteration), and part is
    the best state seen."""
    return _kway_jet(lambda *a: _lib.ek_kway_jet_host(hgr._h, *a), "kway_jet_host", hgr, part, k, eps, bounds,
                     max_iters, patience, neg)


def _kway_rebalance(call, what, hgr, part, k, imbalance, bounds, max_rounds):
    """_kway_refine_w for the rebalancing entries."""
    start = np.ascontiguousarray(part, np.int32)
    if len(start) != hgr.nodes:
        raise ValueError(f"part has {len(start)} entries for {hgr.nodes} nodes")
    if bounds is not None:
        bounds = np.ascontiguousarray(bounds, np.int64)
        if len(bounds) != int(k):
            raise ValueError(f"{len(bounds)} bounds for {k} parts")
    o = KwayRebalanceOpts()
    _lib.ek_kway_rebalance_default_opts(ctypes.byref(o))
    o.k, o.max_rounds, o.imbalance = int(k), int(max_rounds), float(imbalance)
    cap = int(max_rounds) if max_rounds > 0 else 256
    while True:
        out = start.copy()
        log = np.zeros((cap, 4), np.int64)
        r = KwayRebalanceResult()
        _chk(call(ctypes.byref(o), _p(bounds), _p(out), _p(log), cap, ctypes.byref(r)), what)
        if r.rounds <= cap:  # (else: deterministic, so the same run again with room for its log)
            break
        cap = r.rounds
    res = {name: getattr(r, name) for name, _ in KwayRebalanceResult._fields_}
    return out, res, log[:r.rounds].copy()


def kway_rebalance_host(hgr, part, k, eps=0.03, bounds=None, max_rounds=0):
    """k-way rebalancing on the host (ek_kway_rebalance_host, the device path's checker): the nodes of the parts above
    bounds[p] (or above floor((1 + eps) ceil(W / k)) when bounds is None) move to parts with room until no part is
    above its bound or nothing fits.  Returns (part, result dict, round log); a log row is (proposers, evicted nodes,
    moved nodes, the excess after the round).  The weighted connectivity may rise."""
    return _kway_rebalance(lambda *a: _lib.ek_kway_rebalance_host(hgr._h, *a), "kway_rebalance_host", hgr, part, k,
                           eps, bounds, max_rounds)


def _sweep_opts(imbalance, ratio):
    o = SweepOpts()
    _lib.ek_sweep_default_opts(ctypes.byref(o))
    o.objective, o.imbalance = 1 if ratio else 0, float(imbalance)
    return o


def _sweep_result(r):
    return {name: getattr(r, name) for name, _ in SweepResult._fields_}


def _sweep_cut(call, what, hgr, v, imbalance, ratio):
    v = np.ascontiguousarray(v, np.float64)
    if len(v) != hgr.nodes:
        raise ValueError(f"v has {len(v)} entries for {hgr.nodes} nodes")
    o = _sweep_opts(imbalance, ratio)
    order = np.full(len(v), -1, np.int32)
    profile = np.full(len(v) + 1, -1, np.int32)
    r = SweepResult()
    _chk(call(_p(v), ctypes.byref(o), _p(order), _p(profile), ctypes.byref(r)), what)
    return _sweep_result(r), order, profile


def sweep_cut_host(hgr, v, imbalance=0.03, ratio=False):
    """The sweep cut of v over hgr's nets inside the window of L_max = floor((1 + imbalance) ceil(n / 2)), on the
    host (ek_sweep_cut_host, the device path's checker): the minimum cut, or with ratio the ratio cut.
    Returns (result dict, order, profile): order[r] the node at rank r, profile[s] the nets cut by split s."""
    return _sweep_cut(lambda *a: _lib.ek_sweep_cut_host(hgr._h, *a), "sweep_cut_host", hgr, v, imbalance, ratio)


def _sweep_w_result(r):
    return {name: getattr(r, name) for name, _ in SweepWResult._fields_}


def _sweep_cut_w(call, what, hgr, v, imbalance, result_type=None):
    result_type = result_type or SweepWResult
    v = np.ascontiguousarray(v, np.float64)
    if len(v) != hgr.nodes:
        raise ValueError(f"v has {len(v)} entries for {hgr.nodes} nodes")
    o = _sweep_opts(imbalance, False)
    order = np.full(len(v), -1, np.int32)
    profile = np.full(len(v) + 1, -1, np.int64)
    prefix = np.full(len(v) + 1, -1, np.int64)
    r = result_type()
    _chk(call(_p(v), ctypes.byref(o), _p(order), _p(profile), _p(prefix), ctypes.byref(r)), what)
    return {name: getattr(r, name) for name, _ in result_type._fields_}, order, profile, prefix


def sweep_cut_w_host(hgr, v, imbalance=0.03):
    """The weighted sweep cut of v over hgr's nets and weights, on the host (ek_sweep_cut_w_host, the device
    path's checker): the least weighted cut among the splits whose two sides weigh at most L_max = floor((1 +
    imbalance) ceil(W / 2)), or, when there is none (feasible = 0), the split closest to balance.
    Returns (result dict, order, profile_w, prefix): order[r] the node at rank r, profile_w[s] the weight of the
    nets cut by split s, prefix[s] the weight of side 1 of split s (int64 both)."""
    return _sweep_cut_w(lambda *a: _lib.ek_sweep_cut_w_host(hgr._h, *a), "sweep_cut_w_host", hgr, v, imbalance)


def _bounds(bounds):
    b = np.ascontiguousarray(bounds, np.int64)
    if b.shape != (2,):
        raise ValueError("bounds: the two sides' greatest weights (L0, L1)")
    return b


def sweep_cut_wb_host(hgr, v, bounds):
    """sweep_cut_w_host under per-side bounds (ek_sweep_cut_wb_host): side 0 may weigh at most bounds[0], side 1
    (the low ranks) at most bounds[1]; the balance key is the slack difference.  Returns (result dict, order,
    profile_w, prefix)."""
    b = _bounds(bounds)
    return _sweep_cut_w(lambda v_, o, *a: _lib.ek_sweep_cut_wb_host(hgr._h, v_, o, _p(b), *a), "sweep_cut_wb_host", hgr, v,
                        0.0, SweepWBResult)


def fm_refine_wb_host(hgr, side, bounds, max_passes=0, stall=1000, move_cap=None):
    """fm_refine_w_host under per-side bounds (ek_fm_refine_wb_host): side s may hold at most bounds[s]; a pass_log
    row ends with the slack difference.  Returns (side, pass_log, move_log, result dict)."""
    b = _bounds(bounds)
    return _fm_refine(lambda o, *a: _lib.ek_fm_refine_wb_host(hgr._h, o, _p(b), *a), "fm_refine_wb_host", hgr, side, 0.0,
                      max_passes, stall, move_cap, FmWBResult)


def kway_bisect_bounds(Wb, kb, part_bound, mult):
    """(L0, L1) of one bisection of the k-way recursion (ek_kway_bisect_bounds)."""
    out = np.zeros(2, np.int64)
    _chk(_lib.ek_kway_bisect_bounds(int(Wb), int(kb), int(part_bound), float(mult), _p(out)), "kway_bisect_bounds")
    return int(out[0]), int(out[1])


def _kway_metrics_w(call, what, hgr, part, k):
    part = np.ascontiguousarray(part, np.int32)
    if len(part) != hgr.nodes:
        raise ValueError(f"part has {len(part)} entries for {hgr.nodes} nodes")
    out = np.zeros(4 + max(int(k), 0), np.int64)
    _chk(call(_p(part), int(k), _p(out)), what)
    return tuple(int(x) for x in out[:4]), out[4:].copy()


def kway_metrics_w_host(hgr, part, k):
    """((cut nets, connectivity, weighted connectivity, SOED), part weights) of a part vector under hgr's weights
    (ek_kway_metrics_w_host)."""
    return _kway_metrics_w(lambda *a: _lib.ek_kway_metrics_w_host(hgr._h, *a), "kway_metrics_w_host", hgr, part, k)


def _kway_ml_opts(k, imbalance, coarse_nodes, weighted_laplacian, write_results, out_dir, max_passes, stall, lanczos):
    o = KwayMlOpts()
    _lib.ek_kway_ml_default_opts(ctypes.byref(o))
    o.k, o.imbalance, o.flags = int(k), float(imbalance), ML_WEIGHTED_LAPLACIAN if weighted_laplacian else 0
    o.write_results = 1 if write_results else 0
    o.out_dir = os.fsencode(out_dir) if out_dir else None
    o.ml.coarse_nodes, o.ml.fm.max_passes, o.ml.fm.stall = int(coarse_nodes), int(max_passes), int(stall)
    for name, val in (lanczos or {}).items():
        setattr(o.ml.lanczos, name, val)
    return o


def _kway_ml_result(r):
    out = {k: getattr(r, k) for k, _ in KwayMlResult._fields_ if k != "t_level"}
    out["t_level"] = list(r.t_level)
    return out


def _kway_direct_opts(k, eps, host_contract, weighted_laplacian, coarse_nodes, jet, initial, write_results, out_dir):
    """jet: ek_kway_jet_opts fields to override (max_iters, patience, neg_num, neg_den); initial: ek_ml_opts fields of
    the initial partition to override, `fm`, `match` and `lanczos` as dicts of their own fields."""
    o = KwayDirectOpts()
    _lib.ek_kway_direct_default_opts(ctypes.byref(o))
    o.k, o.imbalance, o.coarse_nodes = int(k), float(eps), int(coarse_nodes)
    o.flags = ((KWAY_DIRECT_HOST_CONTRACT if host_contract else 0)
               | (KWAY_DIRECT_WEIGHTED_LAPLACIAN if weighted_laplacian else 0))
    o.write_results = 1 if write_results else 0
    o.out_dir = os.fsencode(out_dir) if out_dir else None
    for name, val in (jet or {}).items():
        setattr(o.jet, name, val)
    for name, val in (initial or {}).items():
        if isinstance(val, dict):
            for sub, x in val.items():
                setattr(getattr(o.initial.ml, name), sub, x)
        else:
            setattr(o.initial.ml, name, val)
    return o


def _kway_direct_result(r):
    out = {k: getattr(r, k) for k in ("k", "levels", "initial_fallbacks", "infeasible_sweeps") + _KWAY_DIRECT_INTS
           + _KWAY_DIRECT_TIMES}
    for k in _KWAY_DIRECT_LEVEL_FIELDS:
        out[k] = list(getattr(r, k))[:r.levels + 1]
    return out


def _fm_refine(call, what, hgr, side, imbalance, max_passes, stall, move_cap, result_type=None):
    """(side, pass_log, move_log, result dict): pass_log has one row per pass run, the last uncounted one
    included, (moves tried, t*, cut, |s0 - s1|); move_log (FM_MOVE_DTYPE) every move tried, in order.
    result_type: the entry's result struct (FmResult by default, FmWResult for the weighted entries)."""
    result_type = result_type or FmResult
    start = np.ascontiguousarray(side, np.uint8)
    if len(start) != hgr.nodes:
        raise ValueError(f"side has {len(start)} entries for {hgr.nodes} nodes")
    o = FmOpts()
    _lib.ek_fm_default_opts(ctypes.byref(o))
    o.imbalance, o.max_passes, o.stall = float(imbalance), int(max_passes), int(stall)
    pass_cap = 64
    move_cap = max(1024, 4 * min(len(start), 1 << 20)) if move_cap is None else max(int(move_cap), 1)
    while True:
        out = start.copy()
        plog = np.zeros((pass_cap, 4), np.int64)
        mlog = np.zeros(move_cap, FM_MOVE_DTYPE)
        r = result_type()
        _chk(call(ctypes.byref(o), _p(out), _p(plog), pass_cap, _p(mlog), move_cap, ctypes.byref(r)), what)
        if r.passes_run <= pass_cap and r.moves_tried <= move_cap:
            break  # (else: deterministic, so the same run again with room for its logs)
        pass_cap, move_cap = max(pass_cap, r.passes_run), max(move_cap, r.moves_tried)
    res = {name: getattr(r, name) for name, _ in result_type._fields_}
    return out, plog[:r.passes_run].copy(), mlog[:r.moves_tried].copy(), res


def fm_refine_host(hgr, side, imbalance=0.03, max_passes=0, stall=1000, move_cap=None):
    """Fiduccia-Mattheyses refinement of a bipartition on the integer net cut under L_max = floor((1 + imbalance)
    ceil(n / 2)), on the host (ek_fm_refine_host, the device path's checker).  Returns (side, pass_log, move_log,
    result dict).  move_cap: room for the move log (default 4 n); a run that tries more moves is run again with
    room for them."""
    return _fm_refine(lambda *a: _lib.ek_fm_refine_host(hgr._h, *a), "fm_refine_host", hgr, side, imbalance,
                      max_passes, stall, move_cap)


def bipart_metrics_host(hgr, side):
    """(weighted cut, cut nets, W0, W1) of a side vector under hgr's weights, 1 where it carries none
    (ek_bipart_metrics_host): only nets of at least 2 distinct pins count, a repeated pin once."""
    side = np.ascontiguousarray(side, np.uint8)
    if len(side) != hgr.nodes:
        raise ValueError(f"side has {len(side)} entries for {hgr.nodes} nodes")
    out = np.zeros(4, np.int64)
    _chk(_lib.ek_bipart_metrics_host(hgr._h, _p(side), _p(out)), "bipart_metrics_host")
    return tuple(int(x) for x in out)


def fm_refine_w_host(hgr, side, imbalance=0.03, max_passes=0, stall=1000, move_cap=None):
    """fm_refine_host under hgr's node and net weights (ek_fm_refine_w_host, the checker of Context.fm_refine_w):
    the weighted cut, L_max = floor((1 + imbalance) ceil(W / 2)) on the sides' weights.  Returns (side, pass_log,
    move_log, result dict): a move's gain and cut are weighted, a pass_log row ends with |S0 - S1|."""
    return _fm_refine(lambda *a: _lib.ek_fm_refine_w_host(hgr._h, *a), "fm_refine_w_host", hgr, side, imbalance,
                      max_passes, stall, move_cap, FmWResult)


def _match(call, what, hgr, max_cluster, max_net, max_rounds):
    """(mate, cluster, round log, result dict): the log has one row per round that matched, (proposers, pairs)."""
    o = MatchOpts()
    _lib.ek_match_default_opts(ctypes.byref(o))
    o.max_net, o.max_rounds, o.max_cluster = int(max_net), int(max_rounds), int(max_cluster)
    n = hgr.nodes
    cap = int(max_rounds) if max_rounds > 0 else 64
    while True:
        mate = np.full(n, -2, np.int32)
        cluster = np.full(n, -2, np.int32)
        log = np.zeros((cap, 2), np.int64)
        r = MatchResult()
        _chk(call(ctypes.byref(o), _p(mate), _p(cluster), _p(log), cap, ctypes.byref(r)), what)
        if r.rounds <= cap:  # (else: deterministic, so the same run again with room for its log)
            break
        cap = r.rounds
    res = {name: getattr(r, name) for name, _ in MatchResult._fields_ if name != "pad"}
    return mate, cluster, log[:r.rounds].copy(), res


def match_host(hgr, max_cluster=2, max_net=64, max_rounds=8):
    """The heavy-edge matching of the coarsening on the host (ek_match_host, the checker of Context.match): pairs
    that propose to each other over their best shared net of at most max_net pins, their weights summing to at most
    max_cluster.  Returns (mate, cluster, round log, result dict): mate[v] the partner or -1, cluster[v] the rank of
    v's cluster among the clusters' least ids."""
    return _match(lambda *a: _lib.ek_match_host(hgr._h, *a), "match_host", hgr, max_cluster, max_net, max_rounds)


def _cluster(call, what, hgr, max_cluster, max_net, max_rounds):
    """(rep, cluster, round log, result dict): the log has one row per round that joined, (proposers, movers, joins)."""
    o = MatchOpts()
    _lib.ek_match_default_opts(ctypes.byref(o))
    o.max_net, o.max_rounds, o.max_cluster = int(max_net), int(max_rounds), int(max_cluster)
    n = hgr.nodes
    cap = int(max_rounds) if max_rounds > 0 else 64
    while True:
        rep = np.full(n, -2, np.int32)
        cluster = np.full(n, -2, np.int32)
        log = np.zeros((cap, 3), np.int64)
        r = ClusterResult()
        _chk(call(ctypes.byref(o), _p(rep), _p(cluster), _p(log), cap, ctypes.byref(r)), what)
        if r.rounds <= cap:  # (else: deterministic, so the same run again with room for its log)
            break
        cap = r.rounds
    res = {name: getattr(r, name) for name, _ in ClusterResult._fields_ if name != "pad"}
    return rep, cluster, log[:r.rounds].copy(), res


def cluster_host(hgr, max_cluster, max_net=64, max_rounds=8):
    """The multi-node clustering of the coarsening on the host (ek_cluster_host, the checker of Context.cluster): a
    single node joins the cluster of its best shared net of at most max_net pins while the cluster's weight stays at
    most max_cluster.  Returns (rep, cluster, round log, result dict): rep[v] the root of v's cluster, cluster[v] the
    rank of that root among the roots."""
    return _cluster(lambda *a: _lib.ek_cluster_host(hgr._h, *a), "cluster_host", hgr, max_cluster, max_net, max_rounds)


def _coarsening(name):
    if name not in _COARSENINGS:
        raise ValueError(f"coarsening {name!r}: one of {sorted(_COARSENINGS)}")
    return _COARSENINGS[name]


def _ml_opts(imbalance, coarse_nodes, max_levels, max_cluster, max_net, max_rounds, max_passes, stall, lanczos):
    o = MlOpts()
    _lib.ek_ml_default_opts(ctypes.byref(o))
    o.imbalance, o.coarse_nodes, o.max_levels = float(imbalance), int(coarse_nodes), int(max_levels)
    o.match.max_cluster, o.match.max_net, o.match.max_rounds = int(max_cluster), int(max_net), int(max_rounds)
    o.fm.max_passes, o.fm.stall = int(max_passes), int(stall)
    for name, val in (lanczos or {}).items():
        setattr(o.lanczos, name, val)
    return o


def _ml_result(r):
    out = {k: getattr(r, k) for k in ("levels", "coarsest_fallback") + _ML_INTS + _ML_TIMES}
    for k in _ML_LEVEL_FIELDS:
        out[k] = list(getattr(r, k))[:r.levels + 1]
    return out


def eig_write(path, lam, median, bits, v):
    bits = np.ascontiguousarray(bits, np.uint8)
    v = np.ascontiguousarray(v, np.float64)
    _chk(_lib.ek_eig_write(os.fsencode(path), len(v), float(lam), float(median), _p(bits), _p(v)), "eig_write")


def eig_read(path, n):
    """pre_saved_EIG file as cKL reads it (cKL.cpp:155-174)."""
    lam, med = ctypes.c_double(), ctypes.c_double()
    bits = np.zeros(n, np.uint8)
    v = np.zeros(n, np.float64)
    o0 = np.empty(n, np.int32)
    o1 = np.empty(n, np.int32)
    n0, n1 = _I64(), _I64()
    _chk(_lib.ek_eig_read(os.fsencode(path), n, ctypes.byref(lam), ctypes.byref(med), _p(bits), _p(v), _p(o0),
                          ctypes.byref(n0), _p(o1), ctypes.byref(n1)), f"eig_read {path}")
    return lam.value, med.value, bits, v, o0[: n0.value].copy(), o1[: n1.value].copy()


def random_split(n, seed):
    """cKL.cpp:176-192 with std::mt19937(seed): (remain[0], remain[1])."""
    o0 = np.empty(n // 2, np.int32)
    o1 = np.empty(n - n // 2, np.int32)
    _chk(_lib.ek_random_split(int(n), int(seed) & 0xFFFFFFFF, _p(o0), _p(o1)), "random_split")
    return o0, o1


def device_count():
    c = ctypes.c_int()
    _lib.ek_device_count(ctypes.byref(c))
    return c.value


def comm_unique_id():
    buf = ctypes.create_string_buffer(128)
    _chk(_lib.ek_comm_unique_id(buf), "comm_unique_id")
    return bytes(buf.raw)


# ---------------------------------------------------------------------------
# GPU side
class Context:
    """One MI355X (gfx950) device: SpMV seam, Lanczos Fiedler solver, KL loop."""

    def __init__(self, device=0):
        self._c = _P()
        _chk(_lib.ek_init(int(device), ctypes.byref(self._c)), "ek_init")
        self.n = 0
        self.nrows = 0

    def close(self):
        if getattr(self, "_c", None):
            _lib.ek_destroy(self._c)
            self._c = None

    def __del__(self):
        self.close()

    def synchronize(self):
        _chk(_lib.ek_synchronize(self._c), "synchronize")

    @property
    def stream(self):
        s = _P()
        _chk(_lib.ek_get_stream(self._c, ctypes.byref(s)), "stream")
        return s.value

    def comm_init(self, nranks, rank, uid):
        """RCCL over xGMI (one process per GPU)."""
        buf = ctypes.create_string_buffer(bytes(uid), 128)
        _chk(_lib.ek_comm_init(self._c, int(nranks), int(rank), buf), "comm_init")

    def comm_init_host(self, nranks, rank, allgather, allreduce):
        """Host-staged exchange (ek_comm_init_host): allgather(send: ndarray) -> ndarray of nranks*len(send),
        allreduce(buf: ndarray) -> None (in-place sum), e.g. over torch.distributed gloo."""
        def ag(_user, send, count, recv):
            try:
                src = np.ctypeslib.as_array(send, shape=(count,))
                dst = np.ctypeslib.as_array(recv, shape=(count * nranks,))
                dst[:] = allgather(src.copy())
                return 0
            except Exception:  # a failed collective must not unwind through C
                import traceback
                traceback.print_exc()
                return 1

        def ar(_user, buf, count):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:
                import traceback
                traceback.print_exc()
                return 1

        self._comm_cbs = (ALLGATHER_FN(ag), ALLREDUCE_FN(ar))  # kept alive with the context
        _chk(_lib.ek_comm_init_host(self._c, int(nranks), int(rank), self._comm_cbs[0], self._comm_cbs[1], None),
             "comm_init_host")

    # SpMV seam (SparseSymMatProd::perform_op, cEIG.cpp:194)
    def spmv_setup(self, n, row0, rowptr, col, val):
        rowptr = np.ascontiguousarray(rowptr, np.int32)
        col = np.ascontiguousarray(col, np.int32)
        val = np.ascontiguousarray(val, np.float64)
        nrows = len(rowptr) - 1
        _chk(_lib.ek_spmv_setup(self._c, int(n), int(row0), nrows, _p(rowptr), _p(col), _p(val)), "spmv_setup")
        self.n, self.nrows = int(n), nrows

    def spmv_setup_pins(self, hgr, weighted=False):
        """This context's Laplacian rows assembled on the GPU from the pins (ek_spmv_setup_pins);
        returns True when the device build ran (False: the host fallback).  weighted: the net-weighted
        Laplacian of Hypergraph.laplacian(weighted=True) (ek_spmv_setup_pins_w; no net weights: NULL, all ones)."""
        net_ptr, pins = hgr.pins()
        dev = ctypes.c_int32(0)
        if weighted:
            net_w = hgr.weights()[1]
            net_w = None if net_w is None else np.ascontiguousarray(net_w, np.int32)
            _chk(_lib.ek_spmv_setup_pins_w(self._c, hgr.nodes, len(net_ptr) - 1, _p(net_ptr), _p(pins),
                                           None if net_w is None else _p(net_w), ctypes.byref(dev)), "spmv_setup_pins_w")
        else:
            _chk(_lib.ek_spmv_setup_pins(self._c, hgr.nodes, len(net_ptr) - 1, _p(net_ptr), _p(pins),
                                         ctypes.byref(dev)), "spmv_setup_pins")
        self.n, _, self.nrows = self.spmv_dims()
        return bool(dev.value)

    def spmv_host(self, x):
        x = np.ascontiguousarray(x, np.float64)
        y = np.empty(self.nrows, np.float64)
        _chk(_lib.ek_spmv_host(self._c, _p(x), _p(y)), "spmv")
        return y

    def spmv_device(self, x_ptr, y_ptr, stream=None):
        _chk(_lib.ek_spmv(self._c, x_ptr, y_ptr, stream), "spmv")

    def spmv_dims(self):
        """(n, row0, nrows) of the rows the context owns (ek_spmv_dims)."""
        n, r0, nr = _I64(), _I64(), _I64()
        _chk(_lib.ek_spmv_dims(self._c, ctypes.byref(n), ctypes.byref(r0), ctypes.byref(nr)), "spmv_dims")
        return n.value, r0.value, nr.value

    def spmv_bytes(self, fused=False):
        """Algorithmic bytes of one SpMV; fused: the Lanczos form (+ f read, basis column write)."""
        return _lib.ek_spmv_bytes(self._c) + (16 * self.spmv_dims()[2] if fused else 0)

    def spmv_format(self, fused=False):
        """(packed, stored bytes per launch): the storage the SpMV reads (ek_spmv_format)."""
        pk, b = ctypes.c_int32(0), _I64(0)
        _chk(_lib.ek_spmv_format(self._c, ctypes.byref(pk), ctypes.byref(b)), "ek_spmv_format")
        return bool(pk.value), int(b.value) + (16 * self.spmv_dims()[2] if fused else 0)

    def spmv_exchange(self):
        """(halo, doubles received, doubles sent) per sharded Lanczos step (ek_spmv_exchange)."""
        hl, rv, sd = ctypes.c_int32(0), _I64(0), _I64(0)
        _chk(_lib.ek_spmv_exchange(self._c, ctypes.byref(hl), ctypes.byref(rv), ctypes.byref(sd)), "ek_spmv_exchange")
        return bool(hl.value), int(rv.value), int(sd.value)

    def comm_stats(self):
        """The sharded solves' exchange accounting since the last setup (ek_comm_stats):
        exchanges of f, point-to-point messages sent / received, and the last timed
        (time_spmv) solve's exchange and all-reduce milliseconds with their counts."""
        e, sd, rv, xt, at = _I64(0), _I64(0), _I64(0), _I64(0), _I64(0)
        xm, am = ctypes.c_double(0.0), ctypes.c_double(0.0)
        _chk(_lib.ek_comm_stats(self._c, ctypes.byref(e), ctypes.byref(sd), ctypes.byref(rv), ctypes.byref(xm),
                                ctypes.byref(xt), ctypes.byref(am), ctypes.byref(at)), "ek_comm_stats")
        return {"exchanges": int(e.value), "sends": int(sd.value), "recvs": int(rv.value),
                "exchange_ms": xm.value, "exchanges_timed": int(xt.value), "allreduce_ms": am.value,
                "allreduces_timed": int(at.value)}

    def spmv_gather_bench(self, iters=200):
        """Average microseconds per launch of the SpMV's gather-only ceiling kernel (ek_spmv_gather_bench)."""
        us = ctypes.c_double()
        _chk(_lib.ek_spmv_gather_bench(self._c, int(iters), ctypes.byref(us)), "spmv_gather_bench")
        return us.value

    def spmv_bench(self, iters=200, fused=True):
        """Average microseconds per back-to-back SpMV launch on resident buffers."""
        us = ctypes.c_double()
        _chk(_lib.ek_spmv_bench(self._c, int(iters), int(fused), ctypes.byref(us)), "spmv_bench")
        return us.value

    def lanczos_fiedler(self, ncv=0, tol=1e-10, maxit=1000, deflate=True, time_spmv=False, reorth=3, check_every=8,
                        basis32=True, alpha_last=False, keep_min=-1, reorth_thresh=0.0):
        """Fiedler pair (Spectra SymEigsSolver(nev=2, ncv=min(100,n/2)), cEIG.cpp:194-207).  check_every: steps
        between mid-cycle convergence tests after the first cycle (0: at cycle ends only, Spectra's schedule).
        basis32: the update reads the basis's fp32 shadow when that is exact to fp64 rounding (ek_lanczos_opts).
        alpha_last: the SpMV's last workgroup reduces alpha (default: every projection workgroup does).
        keep_min: floor on the vectors an implicit restart keeps (-1: ncv/5, 0: Spectra's nev_adjusted alone).
        reorth: 3 partial reorthogonalisation (Simon's omega recurrence, threshold reorth_thresh, <= 0:
        1e-10), 1 full (every step), 2 CGS2."""
        o = LanczosOpts(int(ncv), int(maxit), float(tol), 1 if deflate else 0, 1 if time_spmv else 0, int(reorth),
                        int(check_every), 1 if basis32 else 0, 1 if alpha_last else 0, int(keep_min),
                        float(reorth_thresh))
        st = LanczosStats()
        lam = ctypes.c_double()
        v = np.empty(self.n, np.float64)
        _chk(_lib.ek_lanczos_fiedler(self._c, ctypes.byref(o), ctypes.byref(lam), _p(v), ctypes.byref(st)),
             "lanczos_fiedler")
        return lam.value, v, {k: getattr(st, k) for k, _ in LanczosStats._fields_}

    # KL (cKL.cpp:288-406)
    def kl_graph_setup(self, csr):
        self.kl_n = csr.nrows
        _chk(_lib.ek_kl_graph_setup(self._c, csr.nrows, _p(np.ascontiguousarray(csr.rowptr, np.int32)),
                                    _p(np.ascontiguousarray(csr.col, np.int32)),
                                    _p(np.ascontiguousarray(csr.val, np.float32))), "kl_graph_setup")

    def kl_nets_setup(self, net_ptr, pins):
        net_ptr = np.ascontiguousarray(net_ptr, np.int64)
        pins = np.ascontiguousarray(pins, np.int32)
        _chk(_lib.ek_kl_nets_setup(self._c, len(net_ptr) - 1, _p(net_ptr), _p(pins)), "kl_nets_setup")

    def kl_set_partition(self, order0, order1):
        o0 = np.ascontiguousarray(order0, np.int32)
        o1 = np.ascontiguousarray(order1, np.int32)
        _chk(_lib.ek_kl_set_partition(self._c, _p(o0), len(o0), _p(o1), len(o1)), "kl_set_partition")
        self._n01 = (len(o0), len(o1))

    def kl_set_partition_bits(self, bits):
        """cKL.cpp:155-174 (-EIG): node i to split[bits[i]], ascending node order."""
        bits = np.ascontiguousarray(bits, np.uint8)
        _chk(_lib.ek_kl_set_partition_bits(self._c, len(bits), _p(bits)), "kl_set_partition_bits")
        n1 = int(np.count_nonzero(bits))
        self._n01 = (len(bits) - n1, n1)

    def kl_set_partition_fiedler(self):
        """The -EIG split on the device from the Fiedler vector the last lanczos_fiedler left on this context:
        median and the remain[] lists of median_split + kl_set_partition_bits.  Returns (median, n0, n1)."""
        med = ctypes.c_double()
        n0, n1 = ctypes.c_int64(), ctypes.c_int64()
        _chk(_lib.ek_kl_set_partition_fiedler(self._c, ctypes.byref(med), ctypes.byref(n0), ctypes.byref(n1)),
             "kl_set_partition_fiedler")
        self._n01 = (n0.value, n1.value)
        return med.value, n0.value, n1.value

    def fiedler_set(self, v):
        """Uploads v as this context's Fiedler vector, the state a successful lanczos_fiedler leaves for
        kl_set_partition_fiedler and its rank / sweep kin (ek_fiedler_set).  None passes a null pointer."""
        if v is None:
            return _chk(_lib.ek_fiedler_set(self._c, 1, None), "fiedler_set")
        v =np.ascontiguousarray(v, np.float64)
        _chk(_lib.ek_fiedler_set(self._c, len(v), _p(v)), "fiedler_set")

    def kl_partition_copy(self):
        """What the last kl_set_partition* call left on the device (ek_kl_partition_copy): a dict of order0,
        order1 (the lists' node ids), plist (position in its list, bit 31 on side 1), side, n0 and n1."""
        n0, n1 = ctypes.c_int64(), ctypes.c_int64()
        _chk(_lib.ek_kl_partition_copy(self._c, None, None, None, None, ctypes.byref(n0), ctypes.byref(n1)),
             "kl_partition_copy")
        n = n0.value + n1.value
        out = {"order0": np.empty(n0.value, np.int32), "order1": np.empty(n1.value, np.int32),
               "plist": np.empty(n, np.uint32), "side": np.empty(n, np.uint8)}
        _chk(_lib.ek_kl_partition_copy(self._c, _p(out["order0"]), _p(out["order1"]), _p(out["plist"]),
                                       _p(out["side"]), None, None), "kl_partition_copy")
        out["n0"], out["n1"] = n0.value, n1.value
        return out

    def kl_set_partition_fiedler_rank(self, n1):
        """kl_set_partition_fiedler with the rank split: side 1 gets the n1 nodes rank_split marks in the
        Fiedler vector left on this context (ek_kl_set_partition_fiedler_rank).  Returns (n0, n1)."""
        a, b = ctypes.c_int64(), ctypes.c_int64()
        _chk(_lib.ek_kl_set_partition_fiedler_rank(self._c, int(n1), ctypes.byref(a), ctypes.byref(b)),
             "kl_set_partition_fiedler_rank")
        self._n01 = (a.value, b.value)
        return a.value, b.value

    def sweep_cut(self, hgr, v, imbalance=0.03, ratio=False):
        """sweep_cut_host on the GPU, on an uploaded copy of v (ek_sweep_cut): the same order, profile and
        result integers.  Returns (result dict, order, profile)."""
        return _sweep_cut(lambda *a: _lib.ek_sweep_cut(self._c, hgr._h, *a), "sweep_cut", hgr, v, imbalance, ratio)

    def kl_set_partition_fiedler_sweep(self, hgr, imbalance=0.03, ratio=False):
        """The sweep cut of the Fiedler vector left on this context, then kl_set_partition_fiedler_rank at its
        n1 (ek_kl_set_partition_fiedler_sweep).  Returns the result dict."""
        o = _sweep_opts(imbalance, ratio)
        r = SweepResult()
        _chk(_lib.ek_kl_set_partition_fiedler_sweep(self._c, hgr._h, ctypes.byref(o), ctypes.byref(r)),
             "kl_set_partition_fiedler_sweep")
        self._n01 = (r.n0, r.n1)
        return _sweep_result(r)

    def sweep_cut_w(self, hgr, v, imbalance=0.03):
        """sweep_cut_w_host on the GPU, on an uploaded copy of v (ek_sweep_cut_w): the same order, profile_w,
        prefix and result integers.  Returns (result dict, order, profile_w, prefix)."""
        return _sweep_cut_w(lambda *a: _lib.ek_sweep_cut_w(self._c, hgr._h, *a), "sweep_cut_w", hgr, v, imbalance)

    def kl_set_partition_fiedler_sweep_w(self, hgr, imbalance=0.03):
        """The weighted sweep cut of the Fiedler vector left on this context, then kl_set_partition_fiedler_rank
        at its n1 (ek_kl_set_partition_fiedler_sweep_w).  Returns the result dict."""
        o = _sweep_opts(imbalance, False)
        r = SweepWResult()
        _chk(_lib.ek_kl_set_partition_fiedler_sweep_w(self._c, hgr._h, ctypes.byref(o), ctypes.byref(r)),
             "kl_set_partition_fiedler_sweep_w")
        self._n01 = (r.n0, r.n1)
        return _sweep_w_result(r)

    def sweep_cut_wb(self, hgr, v, bounds):
        """sweep_cut_wb_host on the GPU (ek_sweep_cut_wb): the same order, profile_w, prefix and result integers."""
        b = _bounds(bounds)
        return _sweep_cut_w(lambda v_, o, *a: _lib.ek_sweep_cut_wb(self._c, hgr._h, v_, o, _p(b), *a), "sweep_cut_wb",
                            hgr, v, 0.0, SweepWBResult)

    def fm_refine_wb(self, hgr, side, bounds, max_passes=0, stall=1000, move_cap=None):
        """fm_refine_wb_host on the GPU (ek_fm_refine_wb): the same sides, logs and result integers."""
        b = _bounds(bounds)
        return _fm_refine(lambda o, *a: _lib.ek_fm_refine_wb(self._c, hgr._h, o, _p(b), *a), "fm_refine_wb", hgr, side,
                          0.0, max_passes, stall, move_cap, FmWBResult)

    def multilevel_bipartition_b(self, hgr, bounds, coarse_nodes=512, max_levels=ML_LEVELS, max_cluster=0, max_net=64,
                                 max_rounds=8, max_passes=0, stall=1000, lanczos=None, weighted_laplacian=False):
        """multilevel_bipartition under per-side bounds (ek_multilevel_bipartition_b): side s ends with at most
        bounds[s] when the coarsest sweep is feasible.  Returns (side per node, result dict); max_part reports
        max(bounds)."""
        b = _bounds(bounds)
        o = _ml_opts(0.0, coarse_nodes, max_levels, max_cluster, max_net, max_rounds, max_passes, stall, lanczos)
        side = np.full(hgr.nodes, 255, np.uint8)
        r = MlResult()
        _chk(_lib.ek_multilevel_bipartition_b(self._c, hgr._h, ctypes.byref(o),
                                              ML_WEIGHTED_LAPLACIAN if weighted_laplacian else 0, _p(b), _p(side),
                                              ctypes.byref(r)), "multilevel_bipartition_b")
        return side, _ml_result(r)

    def kway_metrics_w(self, hgr, part, k):
        """kway_metrics_w_host on the GPU (ek_kway_metrics_w)."""
        return _kway_metrics_w(lambda *a: _lib.ek_kway_metrics_w(self._c, hgr._h, *a), "kway_metrics_w", hgr, part, k)

    def partition_kway_ml(self, hgr, k, imbalance=0.03, coarse_nodes=512, weighted_laplacian=False, max_passes=0,
                          stall=1000, lanczos=None):
        """k-way partition by recursive multilevel bisection under per-side weight bounds (ek_partition_kway_ml):
        every part weighs at most floor((1 + imbalance) ceil(W / k)) under unit node weights.  Returns (part id per
        node, result dict)."""
        o = _kway_ml_opts(k, imbalance, coarse_nodes, weighted_laplacian, False, None, max_passes, stall, lanczos)
        part = np.full(hgr.nodes, -1, np.int32)
        r = KwayMlResult()
        _chk(_lib.ek_partition_kway_ml(self._c, hgr._h, ctypes.byref(o), _p(part), ctypes.byref(r)), "partition_kway_ml")
        return part, _kway_ml_result(r)

    def hgr_contract(self, hgr, cluster, n_coarse=None, hash_bits=64):
        """Hypergraph.contract on the GPU (ek_hgr_contract_device): the same hypergraph byte for byte.  hash_bits:
        the low bits of the nets' set signature that group them (1..64); the result does not depend on it."""
        cluster = np.ascontiguousarray(cluster, np.int32)
        if len(cluster) != hgr.nodes:
            raise ValueError(f"cluster has {len(cluster)} entries for {hgr.nodes} nodes")
        if n_coarse is None:
            n_coarse = int(cluster.max()) + 1 if len(cluster) else 0
        o = ContractOpts()
        _lib.ek_contract_default_opts(ctypes.byref(o))
        o.hash_bits = int(hash_bits)
        c = _P()
        _chk(_lib.ek_hgr_contract_device(self._c, hgr._h, _p(cluster), int(n_coarse), ctypes.byref(o), ctypes.byref(c)),
             "hgr_contract")
        return Hypergraph(c)

    def partition_kway_direct(self, hgr, k, eps=0.03, host_contract=False, weighted_laplacian=False, coarse_nodes=0,
                              jet=None, initial=None, coarsening="match", rebalance=False):
        """The direct k-way multilevel partition (ek_partition_kway_direct_ex): one coarsening by matching and
        contraction (on the device; host_contract: on the host, the same hypergraphs), partition_kway_ml of the
        coarsest level, then kway_jet at every level on the way back up, all under floor((1 + eps) ceil(W / k)).
        coarse_nodes 0: max(512, 128 k).  jet / initial: option fields to override (see _kway_direct_opts).
        coarsening: "match" or "cluster" (Context.cluster in place of Context.match; match_rounds and match_pairs of
        the result then hold its rounds and joins).  rebalance: ek_partition_kway_direct_rb, kway_rebalance before the
        Jet refinement of every level that starts above the bound; the result dict then also holds, per level,
        over_before, excess_before, rb_rounds, rb_moves and excess_after, and t_rebalance.
        Returns (part id per node, result dict)."""
        o = _kway_direct_opts(k, eps, host_contract, weighted_laplacian, coarse_nodes, jet, initial, False, None)
        part = np.full(hgr.nodes, -1, np.int32)
        r = KwayDirectResult()
        if rebalance:
            rb = KwayDirectRbResult()
            _chk(_lib.ek_partition_kway_direct_rb(self._c, hgr._h, ctypes.byref(o), _coarsening(coarsening), _p(part),
                                                  ctypes.byref(r), ctypes.byref(rb)), "partition_kway_direct")
            out = _kway_direct_result(r)
            for name in _KWAY_DIRECT_RB_LEVEL_FIELDS:
                out[name] = list(getattr(rb, name))[:r.levels + 1]
            out["t_rebalance"] = rb.t_rebalance
            return part, out
        _chk(_lib.ek_partition_kway_direct_ex(self._c, hgr._h, ctypes.byref(o), _coarsening(coarsening), _p(part),
                                              ctypes.byref(r)), "partition_kway_direct")
        return part, _kway_direct_result(r)

    def partition_kway_direct_file(self, path, k, eps=0.03, host_contract=False, weighted_laplacian=False,
                                   coarse_nodes=0, jet=None, initial=None, write_results=True, out_dir=None,
                                   coarsening="match"):
        """The same on the hMETIS reading of a file; write_results: results/<base>.part.<k> under out_dir
        (ek_partition_kway_direct_file_ex).  Returns (part id per node, result dict)."""
        o = _kway_direct_opts(k, eps, host_contract, weighted_laplacian, coarse_nodes, jet, initial, write_results,
                              out_dir)
        part = np.full(Hypergraph.read_weighted(path).nodes, -1, np.int32)
        r = KwayDirectResult()
        _chk(_lib.ek_partition_kway_direct_file_ex(self._c, os.fsencode(path), ctypes.byref(o), _coarsening(coarsening),
                                                   _p(part), ctypes.byref(r)), f"partition_kway_direct_file {path}")
        return part, _kway_direct_result(r)

    def partition_kway_ml_file(self, path, k, imbalance=0.03, coarse_nodes=512, weighted_laplacian=False,
                               write_results=True, out_dir=None, max_passes=0, stall=1000, lanczos=None):
        """The same on the hMETIS reading of a file; write_results: results/<base>.part.<k> under out_dir
        (ek_partition_kway_ml_file).  Returns (part id per node, result dict)."""
        o = _kway_ml_opts(k, imbalance, coarse_nodes, weighted_laplacian, write_results, out_dir, max_passes, stall,
                          lanczos)
        part = np.full(Hypergraph.read_weighted(path).nodes, -1, np.int32)
        r = KwayMlResult()
        _chk(_lib.ek_partition_kway_ml_file(self._c, os.fsencode(path), ctypes.byref(o), _p(part), ctypes.byref(r)),
             f"partition_kway_ml_file {path}")
        return part, _kway_ml_result(r)

    def rank_split_device(self, v, n1):
        """rank_split run by the device kernels on an uploaded copy of v (ek_rank_split_device)."""
        v = np.ascontiguousarray(v, np.float64)
        bits = np.empty(len(v), np.uint8)
        _chk(_lib.ek_rank_split_device(self._c, len(v), _p(v), int(n1), _p(bits)), "rank_split_device")
        return bits

    def kway_metrics(self, net_ptr, pins, part, k):
        """(cut nets, connectivity, SOED) of a part vector, on the GPU (ek_kway_metrics)."""
        net_ptr = np.ascontiguousarray(net_ptr, np.int64)
        pins = np.ascontiguousarray(pins, np.int32)
        part = np.ascontiguousarray(part, np.int32)
        if len(pins) and int(pins.max()) >= len(part):
            raise ValueError("part is shorter than the pins' node range")
        out = np.zeros(3, np.int64)
        _chk(_lib.ek_kway_metrics(self._c, len(net_ptr) - 1, _p(net_ptr), _p(pins), _p(part), int(k), _p(out)),
             "kway_metrics")
        return tuple(int(x) for x in out)

    def partition_kway(self, hgr, k, min_spectral=32, limit=-1, lanczos=None):
        """k-way partition by recursive spectral bisection (ek_partition_kway).  lanczos: ek_lanczos_opts
        fields to override for every bisection.  Returns (part id per node, result dict)."""
        o = _kway_opts(k, min_spectral, limit, False, None, lanczos)
        part = np.full(hgr.nodes, -1, np.int32)
        r = KwayResult()
        _chk(_lib.ek_partition_kway(self._c, hgr._h, ctypes.byref(o), _p(part), ctypes.byref(r)), "partition_kway")
        return part, _kway_result(r)

    def fm_refine(self, hgr, side, imbalance=0.03, max_passes=0, stall=1000, move_cap=None):
        """fm_refine_host on the GPU (ek_fm_refine): the same sides, logs and result integers.  Returns (side,
        pass_log, move_log, result dict)."""
        return _fm_refine(lambda *a: _lib.ek_fm_refine(self._c, hgr._h, *a), "fm_refine", hgr, side, imbalance,
                          max_passes, stall, move_cap)

    def fm_refine_w(self, hgr, side, imbalance=0.03, max_passes=0, stall=1000, move_cap=None):
        """fm_refine_w_host on the GPU (ek_fm_refine_w): the same sides, logs and result integers.  Returns (side,
        pass_log, move_log, result dict)."""
        return _fm_refine(lambda *a: _lib.ek_fm_refine_w(self._c, hgr._h, *a), "fm_refine_w", hgr, side, imbalance,
                          max_passes, stall, move_cap, FmWResult)

    def kway_refine(self, hgr, part, k, imbalance=0.03, max_rounds=0):
        """kway_refine_host on the GPU (ek_kway_refine): the same part vector, result integers and
        round log.  Returns (part, result dict, round log)."""
        return _kway_refine(lambda *a: _lib.ek_kway_refine(self._c, hgr._h, *a), "kway_refine", hgr, part, k,
                            imbalance, max_rounds)

    def kway_refine_w(self, hgr, part, k, imbalance=0.03, max_rounds=0, bounds=None):
        """kway_refine_w_host on the GPU (ek_kway_refine_w): the same part vector, result integers and
        round log.  Returns (part, result dict, round log)."""
        return _kway_refine_w(lambda *a: _lib.ek_kway_refine_w(self._c, hgr._h, *a), "kway_refine_w", hgr, part, k,
                              imbalance, max_rounds, bounds)

    def kway_jet(self, hgr, part, k, eps=0.03, bounds=None, max_iters=0, patience=12, neg=(1, 4)):
        """kway_jet_host on the GPU (ek_kway_jet): the same part vector, result integers and iteration
        log.  Returns (part, result dict, iteration log)."""
        return _kway_jet(lambda *a: _lib.ek_kway_jet(self._c, hgr._h, *a), "kway_jet", hgr, part, k, eps, bounds,
                         max_iters, patience, neg)

    def kway_rebalance(self, hgr, part, k, eps=0.03, bounds=None, max_rounds=0):
        """kway_rebalance_host on the GPU (ek_kway_rebalance): the same part vector, result integers and round
        log."""
        return _kway_rebalance(lambda *a: _lib.ek_kway_rebalance(self._c, hgr._h, *a), "kway_rebalance", hgr, part, k,
                               eps, bounds, max_rounds)

    def match(self, hgr, max_cluster=2, max_net=64, max_rounds=8):
        """match_host on the GPU (ek_match): the same mate, cluster, round log and result integers."""
        return _match(lambda *a: _lib.ek_match(self._c, hgr._h, *a), "match", hgr, max_cluster, max_net, max_rounds)

    def cluster(self, hgr, max_cluster, max_net=64, max_rounds=8):
        """cluster_host on the GPU (ek_cluster): the same rep, cluster, round log and result integers."""
        return _cluster(lambda *a: _lib.ek_cluster(self._c, hgr._h, *a), "cluster", hgr, max_cluster, max_net,
                        max_rounds)

    def multilevel_bipartition(self, hgr, imbalance=0.03, coarse_nodes=512, max_levels=ML_LEVELS, max_cluster=0,
                               max_net=64, max_rounds=8, max_passes=0, stall=1000, lanczos=None,
                               weighted_laplacian=False):
        """The multilevel bipartition (ek_multilevel_bipartition): matching and contraction down to coarse_nodes
        nodes, the weighted sweep cut of the coarsest level's Fiedler vector, the weighted FM refinement at every
        level.  max_cluster 0: from W, L_max and coarse_nodes.  lanczos: ek_lanczos_opts fields to override.
        weighted_laplacian: the coarsest level's Laplacian carries its net weights (EK_ML_WEIGHTED_LAPLACIAN).
        Returns (side per node, result dict); the per-level lists of the dict hold levels + 1 entries."""
        o = _ml_opts(imbalance, coarse_nodes, max_levels, max_cluster, max_net, max_rounds, max_passes, stall, lanczos)
        side = np.full(hgr.nodes, 255, np.uint8)
        r = MlResult()
        _chk(_lib.ek_multilevel_bipartition_ex(self._c, hgr._h, ctypes.byref(o),
                                               ML_WEIGHTED_LAPLACIAN if weighted_laplacian else 0, _p(side),
                                               ctypes.byref(r)), "multilevel_bipartition")
        return side, _ml_result(r)

    def multilevel_bipartition_file(self, path, imbalance=0.03, coarse_nodes=512, out_dir=None, max_levels=ML_LEVELS,
                                    max_cluster=0, max_net=64, max_rounds=8, max_passes=0, stall=1000, lanczos=None,
                                    weighted_laplacian=False):
        """The same on the hMETIS reading of a file, written to results/<base>.part.2 under out_dir
        (ek_multilevel_bipartition_file).  Returns (side per node, result dict)."""
        o = _ml_opts(imbalance, coarse_nodes, max_levels, max_cluster, max_net, max_rounds, max_passes, stall, lanczos)
        side = np.full(Hypergraph.read_weighted(path).nodes, 255, np.uint8)
        r = MlResult()
        _chk(_lib.ek_multilevel_bipartition_file_ex(self._c, os.fsencode(path), ctypes.byref(o),
                                                    os.fsencode(out_dir) if out_dir else None,
                                                    ML_WEIGHTED_LAPLACIAN if weighted_laplacian else 0, _p(side),
                                                    ctypes.byref(r)), f"multilevel_bipartition_file {path}")
        return side, _ml_result(r)

    def partition_kway_file(self, path, k, min_spectral=32, limit=-1, write_results=True, out_dir=None,
                            lanczos=None):
        """The same from a .hgr file; write_results: results/<base>.part.<k> under out_dir
        (ek_partition_kway_file).  Returns (part id per node, result dict)."""
        o = _kway_opts(k, min_spectral, limit, write_results, out_dir, lanczos)
        nodes = Hypergraph.read(path).nodes
        part = np.full(nodes, -1, np.int32)
        r = KwayResult()
        _chk(_lib.ek_partition_kway_file(self._c, os.fsencode(path), ctypes.byref(o), _p(part), ctypes.byref(r)),
             f"partition_kway_file {path}")
        return part, _kway_result(r)

    def kl_run(self, limit=-1, cap=None):
        cap = min(self._n01) if cap is None else cap
        log = np.zeros(max(cap, 1), SWAP_DTYPE)
        r = KLResult()
        _chk(_lib.ek_kl_run(self._c, int(limit), _p(log), cap, ctypes.byref(r)), "kl_run")
        res = {k: getattr(r, k) for k, _ in KLResult._fields_}
        return log[: min(r.iterations, cap)], res

    def solve_file(self, path, eig=1, seed=0, write_results=True, out_dir=None, limit=-1, sign_ref=None, ncv=0,
                   tol=1e-10, deflate=True, time_spmv=False, log_cap=0, check_every=8, basis32=True, alpha_last=False,
                   keep_min=-1, reorth=3, reorth_thresh=0.0):
        """The whole path, .hgr -> results/ (ek_solve_file).  eig: 1 GPU Fiedler split (gKL2 -EIG), 2 the
        pre_saved_EIG file (cKL -EIG), 0 random split with std::mt19937(seed).  Returns (result dict, swap log)."""
        o = SolveOpts()
        _lib.ek_solve_default_opts(ctypes.byref(o))
        o.eig, o.seed, o.write_results, o.limit = int(eig), int(seed) & 0xFFFFFFFF, 1 if write_results else 0, int(limit)
        o.out_dir = os.fsencode(out_dir) if out_dir else None
        o.sign_ref = os.fsencode(sign_ref) if sign_ref else None
        o.lanczos = LanczosOpts(int(ncv), 1000, float(tol), 1 if deflate else 0, 1 if time_spmv else 0, int(reorth),
                                int(check_every), 1 if basis32 else 0, 1 if alpha_last else 0, int(keep_min),
                                float(reorth_thresh))
        log = np.empty(max(int(log_cap), 1), SWAP_DTYPE)  # the library writes the first `iterations` records
        r = SolveResult()
        _chk(_lib.ek_solve_file(self._c, os.fsencode(path), ctypes.byref(o), _p(log), int(log_cap), ctypes.byref(r)),
             f"solve_file {path}")
        out = {k: getattr(r, k) for k in ("nets", "nodes", "pins", "median") + _SOLVE_TIMES}
        out["lambda"] = r.lambda_
        out["lanczos"] = {k: getattr(r.lanczos, k) for k, _ in LanczosStats._fields_}
        out["kl"] = {k: getattr(r.kl, k) for k, _ in KLResult._fields_}
        self.kl_n = r.nodes  # (kl_sides: the partition this solve left on the context)
        return out, log[: min(int(log_cap), r.kl.iterations)]

    def kl_sides(self, which):
        out = np.empty(self.kl_n, np.uint8)
        _chk(_lib.ek_kl_sides(self._c, int(which), _p(out)), "kl_sides")
        return out


# ---------------------------------------------------------------------------
# drop-in tools, in-process (same argv / CWD semantics as the executables)
def _cli(tool, *args):
    argv = [tool.encode()] + [os.fsencode(str(a)) for a in args]
    arr = (ctypes.c_char_p * len(argv))(*argv)
    return _lib.ek_cli_main(tool.encode(), len(argv), arr)


def cEIG(path, *flags):
    return _cli("cEIG", path, *flags)


def cKL(path, EIG=False, *flags):
    return _cli("cKL", path, *(["-EIG"] if EIG else []), *flags)


def gKL(path, EIG=False, *flags):
    return _cli("gKL", path, *(["-EIG"] if EIG else []), *flags)


def gKL2(path, EIG=False, *flags):
    return _cli("gKL2", path, *(["-EIG"] if EIG else []), *flags)
