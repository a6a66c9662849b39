"""ctypes binding of the C-ABI declared in include/scoary_hip.h.

The HIP library is the product path: if ``libscoary_hip.so`` is missing or the
GPU is absent, everything here raises -- there is no CPU fallback.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# SCOARY_HIP_LIB: an alternative build of the same sources (kernel A/B experiments, tools/ab_lib.sh)
LIB_PATH = os.environ.get("SCOARY_HIP_LIB") or os.path.join(_HERE, "csrc", "libscoary_hip.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "scoary_hip.h")

ABI_VERSION = 11
# scoary_perm_max_strata() / scoary_perm_strata_max_isolates(): what the stratified label generator takes, known
# here so that the command line can refuse a strata file before the library is loaded (load() compares)
PERM_MAX_STRATA = 1024
PERM_STRATA_MAX_ISOLATES = 20479
# scoary_categorical_max_classes(): the classes a categorical trait may have (spec S20), known here for the same reason
CATEGORICAL_MAX_CLASSES = 8
# scoary_score_max_covariates(): the covariates a score test adjusts for (spec S24), known here for the same reason
SCORE_MAX_COVARIATES = 8

_i64, _u64, _i32, _vp, _cp = (ctypes.c_int64, ctypes.c_uint64, ctypes.c_int,
                              ctypes.c_void_p, ctypes.c_char_p)

# name -> (restype, argtypes); mirrors include/scoary_hip.h one to one
SIGNATURES = {
    "scoary_abi_version": (_i32, []),
    "scoary_create": (_i32, [_i32, ctypes.POINTER(_vp)]),
    "scoary_destroy": (None, [_vp]),
    "scoary_last_error": (_cp, [_vp]),
    "scoary_tiled_quads": (_i64, [_i64]),
    "scoary_tiled_genes": (_i64, [_i64]),
    "scoary_tiled_bytes": (_i64, [_i64, _i64]),
    "scoary_row_words": (_i64, [_i64]),
    "scoary_pack_dense": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "scoary_tile_rows": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp]),
    "scoary_counts": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "scoary_counts_traits_per_pass": (_i64, [_i64]),
    "scoary_trait_plan_bytes": (_i64, [_i64, _i64]),
    "scoary_trait_plan": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "scoary_counts_planned": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "scoary_fisher": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
    "scoary_fisher_lists": (_i32, [_vp, _vp, _i64, _i64] + [_vp] * 7),
    "scoary_fisher_chains_bytes": (_i64, [_i64, _i64]),
    "scoary_fisher_chains_capacity": (_i64, []),
    "scoary_fisher_chains_floor": (ctypes.c_double, []),
    "scoary_set_fisher_route": (_i32, [_vp, _i32]),
    "scoary_fisher_lists_chained": (_i32, [_vp, _vp, _i64, _i64, _i64] + [_vp] * 7 + [_i64, _vp]),
    "scoary_fisher_scipy": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "scoary_fisher_scipy_max_isolates": (_i64, []),
    "scoary_perm_generate": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _u64, _vp, _vp]),
    "scoary_permute": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    "scoary_permute_seq": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _vp, _vp,
                                  _vp]),
    "scoary_minp_fill_scratch_bytes": (_i64, [_i64]),
    "scoary_minp_plan": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, ctypes.POINTER(_i64), _vp]),
    "scoary_minp_fill": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp, _vp]),
    "scoary_permute_minp": (_i32, [_vp] * 6 + [_i64] * 6 + [_vp, _vp]),
    "scoary_stepdown_chunks": (_i64, [_vp, _i64, _i64, _i64]),
    "scoary_stepdown_scratch_bytes": (_i64, [_vp, _i64, _i64, _i64, _i64]),
    "scoary_permute_stepdown": (_i32, [_vp] * 8 + [_i64] * 6 + [_vp] * 4),
    "scoary_list_tiles_words": (_i64, [_i64, _i64, _i64]),
    "scoary_list_tile_words": (_i64, [_i64]),
    "scoary_list_params": (_i32, [_i64, _vp]),
    "scoary_list_max_isolates": (_i64, []),
    "scoary_list_segments": (_i64, [_i64]),
    "scoary_perm_generate_tiles": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _u64, _vp,
                                          _vp]),
    "scoary_perm_generate_tiles_range": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _u64, _i64,
                                                _i64, _vp, _vp]),
    "scoary_perm_generate_tiles_bfrag_range": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _i64, _i64, _u64, _i64,
                                                      _i64, _vp, _vp, _vp]),
    "scoary_perm_max_isolates": (_i64, []),
    "scoary_perm_max_strata": (_i32, []),
    "scoary_perm_strata_max_isolates": (_i64, []),
    "scoary_strata_margins": (_i32, [_vp, _vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "scoary_perm_generate_strata": (_i32, [_vp] * 6 + [_i64] * 6 + [_u64, _vp, _vp]),
    "scoary_perm_generate_tiles_strata_range": (_i32, [_vp] * 6 + [_i64] * 6 + [_u64, _i64, _i64, _vp, _vp]),
    "scoary_perm_generate_tiles_strata_bfrag_range": (_i32, [_vp] * 6 + [_i64] * 6 + [_u64, _i64, _i64, _vp, _vp,
                                                                                     _vp]),
    "scoary_cmh_scratch_bytes": (_i64, [_i64]),
    "scoary_cmh": (_i32, [_vp] * 8 + [_i64] * 4 + [_vp] * 10),
    "scoary_cmh_minp_plan": (_i32, [_vp] * 7 + [_i64] * 4 + [_vp] * 3 + [ctypes.POINTER(_i64), _vp]),
    "scoary_cmh_minp_fill": (_i32, [_vp] * 5 + [_i64] * 3 + [_vp, _vp]),
    "scoary_cmh_exact_max_isolates": (_i64, []),
    "scoary_cmh_exact": (_i32, [_vp] * 7 + [_i64] * 4 + [_vp] * 4 + [_i64] + [_vp] * 5),
    "scoary_cmh_exact_odds": (_i32, [_vp] * 7 + [_i64] * 4 + [_vp] * 3 + [_i64, ctypes.c_double] + [_vp] * 5),
    "scoary_cmh_homogeneity": (_i32, [_vp] * 8 + [_i64] * 4 + [_vp] * 7),
    "scoary_ranksum_max_isolates": (_i64, []),
    "scoary_ranksum": (_i32, [_vp] * 5 + [_i64] * 3 + [_vp] * 5),
    "scoary_ranksum_perm_generate": (_i32, [_vp] * 3 + [_i64] * 5 + [_u64, _vp, _vp]),
    "scoary_ranksum_bfrag_bytes": (_i64, [_i64, _i64, _i64]),
    "scoary_ranksum_perm_generate_bfrag": (_i32, [_vp] * 3 + [_i64] * 5 + [_u64, _vp, _vp]),
    "scoary_permute_ranksum": (_i32, [_vp] * 4 + [_i64] * 4 + [_vp, _vp]),
    "scoary_categorical_max_classes": (_i64, []),
    "scoary_categorical": (_i32, [_vp] * 4 + [_i64] * 4 + [_vp] * 6),
    "scoary_permute_categorical": (_i32, [_vp] * 6 + [_i64] * 4 + [_vp, _vp]),
    "scoary_gcmh_form_doubles": (_i64, []),
    "scoary_gcmh": (_i32, [_vp] * 7 + [_i64] * 5 + [_vp] * 10),
    "scoary_permute_gcmh": (_i32, [_vp] * 6 + [_i64] * 4 + [_vp, _vp]),
    "scoary_cat_wy_prepare": (_i32, [_vp] * 3 + [_i64] * 3 + [_vp] * 5),
    "scoary_permute_cat_wy": (_i32, [_vp] * 8 + [_i64] * 4 + [_vp, _vp, _i64, _vp]),
    "scoary_permute_gcmh_wy": (_i32, [_vp] * 6 + [_i64] * 4 + [_vp, _vp, _i64, _vp]),
    "scoary_cat_stepdown_scratch_bytes": (_i64, [_vp] + [_i64] * 5),
    "scoary_cat_stepdown_gather": (_i32, [_vp] * 6 + [_i64] * 3 + [_vp, _vp]),
    "scoary_gcmh_stepdown_gather": (_i32, [_vp] * 5 + [_i64] * 3 + [_vp, _vp]),
    "scoary_permute_cat_stepdown": (_i32, [_vp] * 6 + [_i64] * 5 + [_vp] * 3 + [_i64, _vp]),
    "scoary_permute_gcmh_stepdown": (_i32, [_vp] * 4 + [_i64] * 5 + [_vp] * 3 + [_i64, _vp]),
    "scoary_score_max_covariates": (_i64, []),
    "scoary_score": (_i32, [_vp] * 6 + [_i64] * 5 + [_vp] * 9),
    "scoary_score_spa_max_isolates": (_i64, []),
    "scoary_score_spa_scratch_bytes": (_i64, [_i64, _i64]),
    "scoary_score_spa": (_i32, [_vp] * 11 + [_i64] * 4 + [ctypes.c_double] + [_vp] * 6),
    "scoary_vanelteren": (_i32, [_vp] * 8 + [_i64] * 4 + [_vp] * 7),
    "scoary_vanelteren_perm_generate": (_i32, [_vp] * 4 + [_i64] * 6 + [_u64, _vp, _vp]),
    "scoary_vanelteren_perm_generate_bfrag": (_i32, [_vp] * 4 + [_i64] * 6 + [_u64, _vp, _vp]),
    "scoary_ranksum_var": (_i32, [_vp] * 4 + [_i64] * 3 + [_vp, _vp]),
    "scoary_rank_wy_prepare": (_i32, [_vp] * 3 + [_i64] * 3 + [_vp] * 3),
    "scoary_permute_rank_wy": (_i32, [_vp] * 5 + [_i64] * 5 + [_vp, _vp, _i64, _vp]),
    "scoary_rank_stepdown_scratch_bytes": (_i64, [_vp] + [_i64] * 4),
    "scoary_rank_stepdown_gather": (_i32, [_vp] * 6 + [_i64] * 3 + [_vp, _vp]),
    "scoary_permute_rank_stepdown": (_i32, [_vp] * 3 + [_i64] * 6 + [_vp] * 3 + [_i64, _vp]),
    "scoary_rank_shift_waves": (_i64, [_i64]),
    "scoary_ranksum_shift": (_i32, [_vp] * 7 + [ctypes.c_double] + [_i64] * 3 + [_vp] * 5),
    "scoary_permute_lists_scratch_bytes": (_i64, [_i64, _i64, _i64, _i64]),
    "scoary_permute_lists": (_i32, [_vp, _vp, _vp, _i64] + [_vp] * 8 + [_i64, _i64, _i64, _i64, _vp,
                                                                       _i32, _vp]),
    "scoary_mfma_max_isolates": (_i64, []),
    "scoary_mfma_panels_bytes": (_i64, [_i64, _i64]),
    "scoary_mfma_bfrag_bytes": (_i64, [_i64, _i64, _i64]),
    "scoary_mfma_breakeven_entries": (_i64, []),
    "scoary_mfma_panels_build": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "scoary_set_mfma_route": (_i32, [_vp, _i32]),
    "scoary_mfma_route": (_i64, [_vp, _vp, _i64, _i64, _i64, _i64]),
    "scoary_mfma_plan": (_i32, [_i32, _i64, _i64, _i64, ctypes.POINTER(_i64)]),
    "scoary_permute_hybrid": (_i32, [_vp, _vp, _vp, _i64] + [_vp] * 8 + [_i64, _i64, _i64, _i64, _vp,
                                                                        _i32, _vp, _vp, _i64, _i64, _vp]),
    "scoary_permute_hybrid_bfrag": (_i32, [_vp, _vp, _vp, _i64] + [_vp] * 8 + [_i64, _i64, _i64, _i64, _vp,
                                                                              _i32, _vp, _vp, _i64, _i64, _i32, _vp]),
    "scoary_lists_scratch_bytes": (_i64, [_i64, _i64]),
    "scoary_lists_slack_entries": (_i64, []),
    "scoary_lists_plan": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp,
                                 ctypes.POINTER(_i64), _vp]),
    "scoary_lists_fill": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _vp]),
    "scoary_hamming": (_i32, [_vp, _vp, _vp, _i64, _i64, _vp, _vp]),
    "scoary_upgma_scratch_bytes": (_i64, [_i64]),
    "scoary_upgma": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _vp, _vp]),
    "scoary_gather_bits": (_i32, [_vp, _vp, _i64, _i64, _vp, _i64, _vp, _vp]),
    "scoary_tree_pairs": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "scoary_tree_permute": (_i32, [_vp, _vp, _i64, _i64, _vp, _vp, _i64, _i64, _i64, _vp, _vp,
                                   _vp]),
    "scoary_row_hash": (_i32, [_vp, _vp, _vp, _i64, _i64, _i64, _vp, _vp]),
    "scoary_pack_records": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp]),
    "scoary_gather": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "scoary_graph_begin": (_i32, [_vp, _vp]),
    "scoary_graph_end": (_i32, [_vp, _vp, ctypes.POINTER(_vp)]),
    "scoary_graph_launch": (_i32, [_vp, _vp, _vp]),
    "scoary_graph_destroy": (None, [_vp]),
    "scoary_set_timing": (_i32, [_vp, _i32]),
    "scoary_last_kernel_ms": (_i32, [_vp, _cp, ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


class ScoaryHipError(RuntimeError):
    pass


def load():
    """Load libscoary_hip.so (after torch, so both share one HIP runtime)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ScoaryHipError(
            "HIP extension not built: %s is missing. Run "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "scoary_amd has no CPU fallback." % LIB_PATH)
    try:
        import torch  # noqa: F401  (loads libamdhip64 first; our .so binds to it by SONAME)
    except ImportError:
        pass
    lib = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)     # AttributeError here = header/library drift
        fn.restype = res
        fn.argtypes = args
    got = lib.scoary_abi_version()
    if got != ABI_VERSION:
        raise ScoaryHipError("ABI version mismatch: library %d, binding %d" % (got, ABI_VERSION))
    if (lib.scoary_perm_max_strata(), lib.scoary_perm_strata_max_isolates()) != \
            (PERM_MAX_STRATA, PERM_STRATA_MAX_ISOLATES):
        raise ScoaryHipError("the library's strata limits differ from the binding's")
    if lib.scoary_categorical_max_classes() != CATEGORICAL_MAX_CLASSES:
        raise ScoaryHipError("the library's class limit differs from the binding's")
    if lib.scoary_score_max_covariates() != SCORE_MAX_COVARIATES:
        raise ScoaryHipError("the library's covariate limit differs from the binding's")
    _lib = lib
    return lib
