"""Runtime of the MI355X-native H-DenseFormer hot path (ctypes over libhdf_hip.so)."""
from ._lib import BF16, F32, EXPORTS, HdfError, LIB_PATH, lib  # noqa: F401

_AUGMENT = ("TrainTransform2D", "TrainTransform3D", "augment_2d", "augment_3d", "crop_origin", "flip2d_code", "flip_flags",
            "rotate_degree", "rotate_matrix", "trz_matrix", "erase2d_keep", "gamma2d", "intensity_2d_", "label_bbox_2d",
            "noise2d_flag", "zoom2d_canvas", "zoom_2d", "crop_resize", "resize_3d", "trunc_normalize_")
_SURFACE = ("cal_score", "multi_dice", "multi_hd", "multi_jc", "multi_vs", "surface_scores",
            "asd_from_result", "asd_scores", "cal_asd", "multi_asd")
_COMPONENTS = ("connected_components", "component_table", "component_stats", "keep_largest_component",
               "remove_small_components")
_MORPHOLOGY = ("binary_dilation", "binary_erosion", "binary_opening", "binary_closing", "binary_fill_holes", "morph_class",
               "fill_class_holes")
_LESIONS = ("component_overlap", "match_components", "lesion_wise_scores")
_DETECTION = ("extract_lesion_candidates", "match_candidates", "DetectionEvaluator")
_REGIONS = ("region_measure", "region_stats", "pet_lesion_measures", "region_quantiles", "region_order_stats",
            "region_median")
_INFERENCE = ("cal_steps", "gaussian_tables", "sliding_window_predict", "slice_predict")


def __getattr__(name):
    if name in _INFERENCE:
        from . import inference
        return getattr(inference, name)
    # `from hdf_rt import augment_3d` works, but `import hdf_rt` alone still loads neither torch nor numpy
    if name in _AUGMENT:
        from . import augment
        return getattr(augment, name)
    if name in _SURFACE:
        from . import surface
        return getattr(surface, name)
    if name in _COMPONENTS:
        from . import components
        return getattr(components, name)
    if name in _MORPHOLOGY:
        from . import morphology
        return getattr(morphology, name)
    if name in _LESIONS:
        from . import lesions
        return getattr(lesions, name)
    if name in _DETECTION:
        from . import detection
        return getattr(detection, name)
    if name in _REGIONS:
        from . import regions
        return getattr(regions, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def __dir__():
    return sorted(list(globals()) + list(_AUGMENT) + list(_SURFACE) + list(_COMPONENTS) + list(_MORPHOLOGY) +
                  list(_LESIONS) + list(_DETECTION) + list(_REGIONS) + list(_INFERENCE))
