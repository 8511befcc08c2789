"""The forcing tables of the inverse piecewise kernels, shared by tests/test_gpu_edges.py and tests/test_gpu_folds.py.  Test
infrastructure only; no GPU is touched here."""

# Piecewise instantiations (include/hgwarp.h variant codes): label -> (options, variant with bounds on the high dwords, variant with the
# fp64 bounds).  The ten of test_gpu_parity.DEFAULT_POLICY; the fp64 form of the list-reading k_pw_rows is its one-window instantiation.
PW_KERNELS = {
    "rows4": ({"self_spans": 0, "patch": 0, "tile": 0, "phase": 4, "compact": 0, "min_row_groups": 0}, 104010, 101000),
    "rows_s80": ({"self_spans": 0, "patch": 0, "tile": 0, "phase": 2, "compact": 0, "min_row_groups": 0}, 302010, 101000),
    "rows_self": ({"self_spans": 1, "patch": 0, "tile": 0, "compact": 0, "min_row_groups": 0}, 104011, 101001),
    "rows_self_unsafe": ({"self_spans": 1, "patch": 0, "tile": 0, "compact": 0, "min_row_groups": 0, "safe_spans": 0}, 104011, 101001),
    "rows_self_safe": ({"self_spans": 1, "patch": 0, "tile": 0, "compact": 0, "min_row_groups": 0, "safe_spans": 1}, 104011, 101001),
    "tile_self": ({"self_spans": 1, "patch": 1, "tile": 1, "min_row_groups": 0}, 504011, 504001),
    "patch_self": ({"self_spans": 1, "patch": 1, "tile": 0, "min_row_groups": 0}, 408011, 401001),
    "rows_compact": ({"self_spans": 0, "patch": 0, "tile": 0, "compact": 1, "phase": 2}, 102110, 101100),
    "patch_lists": ({"self_spans": 0, "patch": 1, "tile": 0}, 408010, 401000),
    "rows1": ({"self_spans": 0, "patch": 0, "tile": 0, "phase": 1, "compact": 0}, 101010, 101000),
    "rows_dense": ({"self_spans": 0, "patch": 0, "tile": 0, "compact": 1}, 111110, 111100),        # (mesh "dense" only: 512-slot rows)
}
SELF_LABELS = {"rows_self", "rows_self_unsafe", "rows_self_safe", "tile_self", "patch_self"}

FRAME_SET_KERNELS = ["default", "rows_self_safe", "rows_self_unsafe", "tile_self", "patch_self", "rows4"]
