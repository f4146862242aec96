"""image-feature-extraction_amd -- MI355X (gfx950) per-voxel Hessian feature engine.

Thin ctypes binding of the C-ABI in ``include/ife_hip.h`` (``csrc/libife_hip.so``).
The product is the HIP library and the C++ host mirror under ``host/``; this module
exists so that tests and ``bench.py`` can call the same entry points from Python.

There is no CPU path here: importing works without a GPU (so that the symbol table
can be checked), but creating a :class:`Context` raises when the library or a gfx950
device is missing.

The package directory name contains a hyphen (it mirrors the reference's repository
name); import it with ``importlib.import_module("image-feature-extraction_amd")``.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# IFE_HIP_LIB selects another build of the same library (kernel tuning experiments)
LIB_PATH = os.environ.get("IFE_HIP_LIB") or os.path.join(_HERE, "csrc", "libife_hip.so")

# enums of include/ife_hip.h
OK, E_ARG, E_SIZE, E_HIP, E_NOMEM, E_STATE = 0, -1, -2, -3, -4, -5
F32, I16, U8, U16 = 0, 1, 2, 3
INTERLEAVED, PLANAR = 0, 1
MEM_HOST, MEM_DEVICE = 0, 1
OPT_TRIG_MODE, OPT_DSCALE_MODE, OPT_PROFILE, OPT_ZCHUNK, OPT_IIR_BLOCK, OPT_IIR_CKPT, OPT_IIR_FMA = 1, 2, 3, 4, 5, 6, 7
OPT_FUSED_DIVIDE = 8
OPT_CONST_LINES = 9
OPT_FEAT_RING = 10
OPT_DENSE_SCRATCH_MB = 11
OPT_Z_SWEEP = 12
OPT_DIFFERENTIAL = 13  # 1: the composite calls take their features from the jet (include/ife_hip.h)
INTERP_LINEAR, INTERP_NEAREST = 0, 1  # ife_interp: interpolation of ife_resample
BSPLINE_MAX_ORDER = 5  # ife_bspline_coefficients / ife_resample_bspline: orders 0 .. 5
BAG_COUNTS, BAG_FREQUENCIES = 0, 1  # ife_bag_values: what the dense bag stream delivers
SS_LAPLACIAN, SS_TUBE, SS_PLATE, SS_BLOB = 0, 1, 2, 3  # ife_scale_measure_kind: measures of ife_scale_select
SS_MAX_MEASURES = 4  # IFE_SS_MAX_MEASURES
SS_MAX_SIGMAS = 255  # scale index 255 says "no scale"
SS_KIND_NAMES = ("laplacian", "tube", "plate", "blob")
Z_STATE_BYTES = 32   # IFE_Z_STATE_BYTES: one state record of the slab Z pass, per line and job
Z_OVERLAP_LO, Z_OVERLAP_HI = 3, 4  # IFE_Z_OVERLAP_*: neighbour planes around a slab's input
NUM_FEATURES = 8
MAX_KERNEL_KINDS = 24  # IFE_MAX_KERNEL_KINDS
FEATURE_NAMES = ("GaussianBlur", "GradientMagnitude", "Eigenvalue1", "Eigenvalue2",
                 "Eigenvalue3", "LaplacianOfGaussian", "GaussianCurvature", "FrobeniusNorm")

# every symbol include/ife_hip.h declares
EXPORTS = (
    "ife_abi_version", "ife_ctx_create", "ife_ctx_destroy", "ife_last_error",
    "ife_ctx_set_stream", "ife_ctx_set_option", "ife_ctx_reserve", "ife_ctx_synchronize",
    "ife_eigenvalues", "ife_eigenvalue_features", "ife_hessian3d", "ife_gradient_magnitude",
    "ife_normalized_gaussian_convolution", "ife_differential_normalized_convolution",
    "ife_emphysema_features",
    "ife_emphysema_features_begin", "ife_emphysema_features_fetch", "ife_emphysema_features_end",
    "ife_fd_hessian_features", "ife_fd_gradient_features", "ife_mask_image_f64",
    "ife_get_kernel_times", "ife_reset_kernel_times", "ife_measure_stream",
    "ife_stage_prepare", "ife_stage_recursive_gaussian", "ife_stage_recursive_gaussian_batch",
    "ife_stage_features", "ife_stage_z_ck_bytes", "ife_stage_z_sweep", "ife_stage_z_combine",
    "ife_stage_z_fused", "ife_stage_recursive_gaussian_quotient",
    "ife_multi_create", "ife_multi_destroy", "ife_multi_last_error", "ife_multi_set_option",
    "ife_multi_emphysema_features", "ife_multi_emphysema_features_begin",
    "ife_multi_emphysema_features_fetch", "ife_multi_emphysema_features_end",
    "ife_sort_f32", "ife_equalized_edges_f32", "ife_equalized_edges_f64", "ife_dense_histogram_f32", "ife_roi_histograms", "ife_bag_image",
    "ife_dense_rois", "ife_dense_roi_histograms", "ife_bag_image_dense",
    "ife_bag_dense_stream_begin", "ife_bag_dense_stream_next", "ife_bag_dense_stream_end",
    "ife_roi_labels", "ife_dense_roi_labels",
    "ife_samples_create", "ife_samples_destroy", "ife_samples_count", "ife_samples_clear",
    "ife_samples_add_features", "ife_samples_add_image", "ife_samples_sort",
    "ife_samples_equalized_edges", "ife_samples_read_column",
    "ife_signed_distance_map", "ife_expected_distance",
    "ife_stage_recursive_gaussian_order", "ife_normalized_convolution_jet", "ife_differential_features",
    "ife_deflate_bound", "ife_deflate", "ife_emphysema_features_fetch_deflated",
    "ife_stage_z_sweep_order", "ife_stage_z_combine_order", "ife_stage_z_fused_order",
    "ife_stage_jet_features", "ife_multi_differential_features", "ife_multi_differential_features_begin",
    "ife_resample", "ife_resample_f64",
    "ife_bspline_coefficients", "ife_bspline_coefficients_f64", "ife_resample_bspline",
    "ife_resample_bspline_f64", "ife_window_u8",
    "ife_mask_bounding_box", "ife_extract_region", "ife_label_membership",
    "ife_device_alloc", "ife_device_upload", "ife_device_free",
    "ife_sample_positions", "ife_random_rois", "ife_extract_rois",
    "ife_value_census_f32", "ife_threshold_mask", "ife_roi_coverage",
    "ife_scale_select",
)


class VolumeDesc(C.Structure):
    _fields_ = [("nx", C.c_int64), ("ny", C.c_int64), ("nz", C.c_int64),
                ("sx", C.c_double), ("sy", C.c_double), ("sz", C.c_double)]


class KernelTime(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_int64), ("total_ms", C.c_double)]


class ScaleMeasure(C.Structure):
    """ife_scale_measure: kind SS_*, polarity +1 (bright) or -1 (dark), gamma of the scale
    normalisation, and alpha, beta, c of the three Frangi kinds (SS_LAPLACIAN ignores them)."""
    _fields_ = [("kind", C.c_int32), ("polarity", C.c_int32), ("gamma", C.c_float), ("alpha", C.c_float),
                ("beta", C.c_float), ("c", C.c_float)]

    def __init__(self, kind=SS_LAPLACIAN, polarity=1, gamma=1.0, alpha=0.5, beta=0.5, c=1.0):
        if isinstance(kind, str):
            if kind not in SS_KIND_NAMES:
                raise ValueError("kind must be one of %s" % (SS_KIND_NAMES,))
            kind = SS_KIND_NAMES.index(kind)
        super().__init__(int(kind), int(polarity), float(gamma), float(alpha), float(beta), float(c))


class IfeError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ife error %d: %s" % (code, msg))
        self.code = code


_lib = None


def load_library():
    """dlopen csrc/libife_hip.so.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "%s is missing: build it with `make -C %s` (hipcc --offload-arch=gfx950); "
            "there is no CPU fallback" % (LIB_PATH, os.path.dirname(LIB_PATH)))
    # A torch wheel carries its own HIP runtime under the same SONAME as the system one this
    # library links to, and whichever copy is loaded first serves the whole process.  Ours
    # first leaves torch on a runtime it was not built for ("No HIP GPUs are available" at its
    # first CUDA call), so where torch is installed it is imported before the library.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(LIB_PATH)
    vp, i32, i64, f32p = C.c_void_p, C.c_int, C.c_int64, C.c_void_p
    vd = C.POINTER(VolumeDesc)
    lib.ife_abi_version.restype = i32
    lib.ife_ctx_create.argtypes = [i32, C.POINTER(vp)]
    lib.ife_ctx_destroy.argtypes = [vp]
    lib.ife_ctx_destroy.restype = None
    lib.ife_last_error.argtypes = [vp]
    lib.ife_last_error.restype = C.c_char_p
    lib.ife_ctx_set_stream.argtypes = [vp, vp]
    lib.ife_ctx_set_option.argtypes = [vp, i32, i32]
    lib.ife_ctx_reserve.argtypes = [vp, vd]
    lib.ife_ctx_synchronize.argtypes = [vp]
    lib.ife_eigenvalues.argtypes = [vp, f32p, i64, f32p, i32]
    lib.ife_eigenvalue_features.argtypes = [vp, f32p, i64, f32p, i32]
    lib.ife_hessian3d.argtypes = [vp, f32p, vd, f32p, i32, i32]
    lib.ife_gradient_magnitude.argtypes = [vp, f32p, vd, f32p, i32]
    lib.ife_normalized_gaussian_convolution.argtypes = [vp, f32p, f32p, vd, C.c_double, f32p, i32]
    lib.ife_differential_normalized_convolution.argtypes = [vp, f32p, f32p, vd, C.c_double, i32, f32p, i32]
    lib.ife_emphysema_features.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32,
                                           f32p, i32, i32]
    lib.ife_emphysema_features_begin.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32, i32]
    lib.ife_emphysema_features_fetch.argtypes = [vp, i32, f32p]
    lib.ife_emphysema_features_end.argtypes = [vp]
    lib.ife_fd_hessian_features.argtypes = [vp, vp, i32, vp, i32, vd, f32p, i32, i32]
    lib.ife_fd_gradient_features.argtypes = [vp, f32p, f32p, vd, f32p, i32]
    lib.ife_mask_image_f64.argtypes = [vp, vp, vp, C.c_double, i64, vp, i32]
    lib.ife_stage_prepare.argtypes = [vp, vp, i32, vp, i32, vd, i32, vp, vp]
    lib.ife_stage_recursive_gaussian.argtypes = [vp, vp, vp, vd, i32, C.c_double]
    lib.ife_stage_recursive_gaussian_batch.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), vd,
                                                       i32, C.POINTER(C.c_double), i32]
    lib.ife_stage_features.argtypes = [vp, vp, vp, vp, i32, vd, i32, i32, vp, i32]
    lib.ife_stage_z_ck_bytes.argtypes = [vd]
    lib.ife_stage_z_ck_bytes.restype = C.c_size_t
    lib.ife_stage_z_sweep.argtypes = [vp, i32, i32, C.POINTER(vp), vd, i64, i64,
                                      C.POINTER(C.c_double), i32, vp, vp, C.POINTER(vp)]
    lib.ife_stage_z_combine.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), vd, i64, i64,
                                        C.POINTER(C.c_double), i32, i32, C.POINTER(vp)]
    lib.ife_stage_z_fused.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(vp), vd, i64, i64,
                                      C.POINTER(C.c_double), i32, i32, vp, vp, C.POINTER(vp)]
    lib.ife_stage_z_sweep_order.argtypes = [vp, i32, i32, C.POINTER(vp), vd, i64, i64,
                                            C.POINTER(C.c_double), C.POINTER(i32), i32, vp, vp, C.POINTER(vp)]
    lib.ife_stage_z_combine_order.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), vd, i64, i64,
                                              C.POINTER(C.c_double), C.POINTER(i32), i32, i32, C.POINTER(vp)]
    lib.ife_stage_z_fused_order.argtypes = [vp, i32, i32, C.POINTER(vp), C.POINTER(vp), vd, i64, i64,
                                            C.POINTER(C.c_double), C.POINTER(i32), i32, i32, vp, vp, C.POINTER(vp)]
    lib.ife_stage_jet_features.argtypes = [vp, C.POINTER(vp), vp, i32, vd, C.c_double, vp, i32]
    lib.ife_stage_recursive_gaussian_quotient.argtypes = [vp, i32, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp),
                                                          vd, i32, C.POINTER(C.c_double)]
    lib.ife_multi_create.argtypes = [C.POINTER(i32), i32, C.POINTER(vp)]
    lib.ife_multi_destroy.argtypes = [vp]
    lib.ife_multi_destroy.restype = None
    lib.ife_multi_last_error.argtypes = [vp]
    lib.ife_multi_last_error.restype = C.c_char_p
    lib.ife_multi_set_option.argtypes = [vp, i32, i32]
    lib.ife_multi_emphysema_features.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32, f32p, i32]
    lib.ife_multi_emphysema_features_begin.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32, i32]
    lib.ife_multi_emphysema_features_fetch.argtypes = [vp, i32, f32p]
    lib.ife_multi_emphysema_features_end.argtypes = [vp]
    lib.ife_multi_differential_features.argtypes = lib.ife_multi_emphysema_features.argtypes
    lib.ife_multi_differential_features_begin.argtypes = lib.ife_multi_emphysema_features_begin.argtypes
    lib.ife_get_kernel_times.argtypes = [vp, C.POINTER(KernelTime), i32]
    lib.ife_reset_kernel_times.argtypes = [vp]
    lib.ife_measure_stream.argtypes = [vp, i32, vp, vp, C.c_size_t, i32, C.POINTER(C.c_double)]
    lib.ife_sort_f32.argtypes = [vp, vp, i64, vp, i32]
    lib.ife_equalized_edges_f32.argtypes = [vp, vp, i64, i32, vp, i32]
    lib.ife_equalized_edges_f64.argtypes = [vp, vp, i64, i32, vp, i32]
    lib.ife_dense_histogram_f32.argtypes = [vp, vp, i32, vp, i64, vp, i32]
    lib.ife_roi_histograms.argtypes = [vp, vp, i32, i32, vp, i32, vd, vp, i32, vp, i32, vp, i32]
    lib.ife_bag_image.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32, vp, i32, vp,
                                  i32, vp, i32]
    lib.ife_dense_rois.argtypes = [vp, vp, i32, vd, C.POINTER(i64), C.POINTER(i64), vp, i64, i32]
    lib.ife_dense_roi_histograms.argtypes = [vp, vp, i32, i32, vp, i32, vp, i32, vd, C.POINTER(i64), vp,
                                             i32, vp, i64, C.POINTER(i64), i32]
    lib.ife_bag_image_dense.argtypes = [vp, vp, i32, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32,
                                        C.POINTER(i64), vp, i32, vp, i64, C.POINTER(i64), i32]
    lib.ife_bag_dense_stream_begin.argtypes = [vp, vp, i32, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32,
                                               C.POINTER(i64), vp, i32, i32, i32, C.POINTER(i64),
                                               C.POINTER(i64), i32]
    lib.ife_bag_dense_stream_next.argtypes = [vp, vp, i64, C.POINTER(i64), C.POINTER(i64)]
    lib.ife_bag_dense_stream_end.argtypes = [vp]
    lib.ife_roi_labels.argtypes = [vp, vp, i32, vd, vp, i64, C.POINTER(i32), i32, i32, vp, i32]
    lib.ife_dense_roi_labels.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(i64), C.POINTER(i32), i32, i32, vp,
                                         i64, C.POINTER(i64), i32]
    lib.ife_samples_create.argtypes = [vp, i32, C.POINTER(vp)]
    lib.ife_samples_destroy.argtypes = [vp]
    lib.ife_samples_destroy.restype = None
    lib.ife_samples_count.argtypes = [vp, i32, C.POINTER(i64)]
    lib.ife_samples_clear.argtypes = [vp]
    lib.ife_samples_add_features.argtypes = [vp, vp, i32, vp, i32, i32, vp, i32, i64, vp, i32,
                                             vp, i64, i32]
    lib.ife_samples_add_image.argtypes = [vp, vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float),
                                          i32, vp, i32, vp, i64, i32]
    lib.ife_samples_sort.argtypes = [vp, vp]
    lib.ife_samples_equalized_edges.argtypes = [vp, vp, i32, vp]
    lib.ife_samples_read_column.argtypes = [vp, vp, i32, vp, i64]
    lib.ife_signed_distance_map.argtypes = [vp, vp, i32, vd, i32, i32, vp, i32]
    lib.ife_expected_distance.argtypes = [vp, vp, i32, vp, vd, C.POINTER(C.c_double),
                                          C.POINTER(i64), i32]
    lib.ife_stage_recursive_gaussian_order.argtypes = [vp, vp, vp, vd, i32, C.c_double, i32]
    lib.ife_normalized_convolution_jet.argtypes = [vp, f32p, f32p, vd, C.c_double, f32p, i32, i32]
    lib.ife_differential_features.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32,
                                              f32p, i32, i32]
    lib.ife_deflate_bound.argtypes = [C.c_size_t]
    lib.ife_deflate_bound.restype = C.c_size_t
    lib.ife_deflate.argtypes = [vp, vp, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                C.POINTER(C.c_uint32), i32]
    lib.ife_emphysema_features_fetch_deflated.argtypes = [vp, i32, i32, vp, C.c_size_t,
                                                          C.POINTER(C.c_size_t), C.POINTER(C.c_uint32)]
    d3 = C.POINTER(C.c_double)
    lib.ife_resample.argtypes = [vp, vp, i32, vd, d3, vd, d3, d3, i32, C.c_double, vp, i32]
    lib.ife_resample_f64.argtypes = [vp, vp, vd, d3, vd, d3, d3, i32, C.c_double, vp, i32]
    lib.ife_bspline_coefficients.argtypes = [vp, vp, i32, vd, i32, vp, i32]
    lib.ife_bspline_coefficients_f64.argtypes = [vp, vp, vd, i32, vp, i32]
    lib.ife_resample_bspline.argtypes = [vp, vp, i32, vd, d3, vd, d3, d3, i32, i32, C.c_double, vp, i32]
    lib.ife_resample_bspline_f64.argtypes = [vp, vp, vd, d3, vd, d3, d3, i32, i32, C.c_double, vp, i32]
    lib.ife_window_u8.argtypes = [vp, vp, vp, C.c_int64, C.c_double, C.c_double, C.c_uint8, C.c_uint8, vp, i32]
    lib.ife_mask_bounding_box.argtypes = [vp, vp, i32, vd, C.POINTER(i64), C.POINTER(i64), i32]
    lib.ife_extract_region.argtypes = [vp, vp, i32, vd, C.POINTER(i64), i32, vp, vp, i32, i32]
    lib.ife_label_membership.argtypes = [vp, vp, i32, i64, C.POINTER(i32), i32, i32, i32, vp, i32]
    lib.ife_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    lib.ife_device_upload.argtypes = [vp, vp, vp, C.c_size_t]
    lib.ife_device_free.argtypes = [vp, vp]
    draw = [vp, vp, i32, vd, C.POINTER(i32), i32, i32, C.POINTER(i64), C.c_uint64, C.c_uint32, C.c_uint64, i64, vp,
            C.POINTER(i64), i32]
    lib.ife_sample_positions.argtypes = draw
    lib.ife_random_rois.argtypes = draw
    lib.ife_extract_rois.argtypes = [vp, vp, i32, vd, vp, i64, vp, i32]
    lib.ife_value_census_f32.argtypes = [vp, vp, i64, vp, vp, i64, C.POINTER(i64), C.POINTER(i64), i32]
    lib.ife_threshold_mask.argtypes = [vp, vp, i64, C.c_float, C.c_float, vp, C.POINTER(i64), i32]
    lib.ife_roi_coverage.argtypes = [vp, vp, i32, vd, vp, i64, C.POINTER(i64), i32, C.POINTER(i64), C.POINTER(i64),
                                     C.POINTER(i64), i32]
    lib.ife_scale_select.argtypes = [vp, vp, i32, vp, i32, vd, C.POINTER(C.c_float), i32, C.POINTER(ScaleMeasure), i32,
                                     vp, vp, i32]
    _lib = lib
    return lib


def _desc(shape_zyx, spacing_xyz):
    nz, ny, nx = (int(v) for v in shape_zyx)
    sx, sy, sz = (float(v) for v in spacing_xyz)
    return VolumeDesc(nx, ny, nz, sx, sy, sz)


_IMG_DT = {np.dtype(np.float32): F32, np.dtype(np.int16): I16}
_MSK_DT = {np.dtype(np.uint8): U8, np.dtype(np.uint16): U16}
_RESAMPLE_DT = {**_IMG_DT, **_MSK_DT}   # what ife_resample reads; float64 goes to ife_resample_f64


def _image_arg(image):
    """The image as a contiguous array of a dtype the library reads (anything else as float32),
    and its dtype code."""
    image = np.ascontiguousarray(image)
    if image.dtype not in _IMG_DT:
        image = image.astype(np.float32)
    return image, _IMG_DT[image.dtype]


def _mask_arg(mask):
    """(contiguous mask, dtype code, pointer); (None, U8, None) without a mask.  The caller keeps
    the array alive across the call."""
    if mask is None:
        return None, U8, None
    mask = np.ascontiguousarray(mask)
    if mask.dtype not in _MSK_DT:
        raise TypeError("mask must be uint8 or uint16")
    return mask, _MSK_DT[mask.dtype], mask.ctypes.data


def _sigma_arg(sigmas):
    return (C.c_float * len(sigmas))(*[float(s) for s in sigmas])


def _size_arg(size_xyz):
    sx, sy, sz = (int(v) for v in size_xyz)
    return (C.c_int64 * 3)(sx, sy, sz)


def _labels_arg(labels):
    """The label volume as a contiguous uint8 array (ExtractLabels reads unsigned char)."""
    labels = np.ascontiguousarray(labels)
    if labels.dtype != np.uint8:
        raise TypeError("labels must be uint8")
    if labels.ndim != 3:
        raise ValueError("labels must be a (z, y, x) volume")
    return labels


def _ignore_arg(ignore):
    """(int array or None, count) of the ignored labels; the library checks their range."""
    ignore = [int(v) for v in ignore]
    return ((C.c_int * len(ignore))(*ignore) if ignore else None), len(ignore)


_BOX_DT = {**_RESAMPLE_DT}   # what ife_mask_bounding_box reads


def _region_arg(index_xyz, size_xyz, flip, elem_bytes, src_shape_zyx, has_pad):
    """(region[6], flip bits) of ife_extract_region, with the refusals that need no device."""
    ix, iy, iz = (int(v) for v in index_xyz)
    sx, sy, sz = (int(v) for v in size_xyz)
    if elem_bytes not in (1, 2, 4, 8):
        raise TypeError("elements of 1, 2, 4 or 8 bytes are copied (got %d)" % elem_bytes)
    if min(sx, sy, sz) < 1:
        raise ValueError("the region's size must be at least 1 on every axis")
    if isinstance(flip, (int, np.integer)) and not isinstance(flip, (bool, np.bool_)):
        bits = int(flip)
        if not 0 <= bits <= 7:
            raise ValueError("flip must be 0 .. 7 (bit a flips axis a) or three booleans (x, y, z)")
    else:
        fx, fy, fz = (bool(v) for v in flip)
        bits = int(fx) | int(fy) << 1 | int(fz) << 2
    nz, ny, nx = (int(v) for v in src_shape_zyx)
    inside = all(i >= 0 and i + s <= n for i, s, n in ((ix, sx, nx), (iy, sy, ny), (iz, sz, nz)))
    if not inside and not has_pad:
        raise ValueError("the region reaches outside the source: a pad_value is required")
    return (C.c_int64 * 6)(ix, iy, iz, sx, sy, sz), bits


def _include_arg(include, inside, outside, dtype):
    """(int array or None, count) of a label set, with the range refusals of ife_label_membership."""
    top = int(np.iinfo(dtype).max)
    include = [int(v) for v in include]
    for name, v in [("include", v) for v in include] + [("inside", int(inside)), ("outside", int(outside))]:
        if not 0 <= v <= top:
            raise ValueError("%s value %d is outside 0 .. %d" % (name, v, top))
    return ((C.c_int * len(include))(*include) if include else None), len(include)


def _draw_args(values, per_value, size_xyz, seed, stream, first_draw, n_draws, dtype):
    """The scalar arguments of ife_sample_positions / ife_random_rois from values to n_draws, and
    the number of sets, with the refusals that need no device."""
    top = 255 if dtype == U8 else 65535
    values = [int(v) for v in values]
    if len(values) > 32:
        raise ValueError("at most 32 values (got %d)" % len(values))
    for v in values:
        if not 0 <= v <= top:
            raise ValueError("value %d is outside 0 .. %d" % (v, top))
    if per_value and not values:
        raise ValueError("per_value needs at least one value")
    size = _size_arg(size_xyz)
    if min(size) < 1:
        raise ValueError("the box size must be at least 1 along every axis")
    if int(n_draws) < 0:
        raise ValueError("negative count")
    for name, v, bits in (("seed", seed, 64), ("stream", stream, 32), ("first_draw", first_draw, 64)):
        if not 0 <= int(v) < 1 << bits:
            raise ValueError("%s must be an unsigned %d-bit number" % (name, bits))
    arr = (C.c_int * len(values))(*values) if values else None
    return (arr, len(values), 1 if per_value else 0, size, int(seed), int(stream), int(first_draw),
            int(n_draws)), (len(values) if per_value else 1)


def _draw_host(ctx, name, width, mask, n_draws, size, values, per_value, seed, stream, first_draw):
    """Context.sample_positions (width ()) and Context.random_rois (width (6,)) on host arrays."""
    mask, mdt, mptr = _mask_arg(mask)
    if mask is None or mask.ndim != 3:
        raise ValueError("mask must be a (z, y, x) volume")
    args, n_sets = _draw_args(values, per_value, size, seed, stream, first_draw, n_draws, mdt)
    out = np.empty((n_sets, int(n_draws)) + width, np.int64)
    counts = Context._draw(ctx, name, mptr, mdt, mask.shape, out.ctypes.data if out.size else None, MEM_HOST, args,
                           n_sets)
    return out, counts


def _threshold_args(low, high):
    """The bounds of ife_threshold_mask as the float32 values the library compares with, and the
    refusals that need no device."""
    low, high = np.float32(low), np.float32(high)
    if np.isnan(low) or np.isnan(high):
        raise ValueError("a threshold is not a number")
    if low > high:
        raise ValueError("Lower threshold cannot be greater than upper threshold.")
    return C.c_float(float(low)), C.c_float(float(high))


def _scale_measures_arg(measures, n_sigmas):
    """The measures of ife_scale_select as a ctypes array, refused as the library refuses them."""
    measures = list(measures)
    if not 1 <= len(measures) <= SS_MAX_MEASURES:
        raise ValueError("n_measures must lie in 1 .. %d" % SS_MAX_MEASURES)
    if n_sigmas > SS_MAX_SIGMAS:
        raise ValueError("n_sigmas must be at most %d" % SS_MAX_SIGMAS)
    arr = (ScaleMeasure * len(measures))()
    for k, m in enumerate(measures):
        if not isinstance(m, ScaleMeasure):
            m = ScaleMeasure(**m) if isinstance(m, dict) else ScaleMeasure(*m)
        if m.kind not in (SS_LAPLACIAN, SS_TUBE, SS_PLATE, SS_BLOB):
            raise ValueError("measures[%d]: kind is not a measure kind" % k)
        if m.polarity not in (1, -1):
            raise ValueError("measures[%d]: polarity must be +1 or -1" % k)
        if not (m.gamma >= 0 and np.isfinite(m.gamma)):
            raise ValueError("measures[%d]: gamma must be finite and not negative" % k)
        if m.kind != SS_LAPLACIAN:
            for name in ("alpha", "beta", "c"):
                v = getattr(m, name)
                if not (v > 0 and np.isfinite(v)):
                    raise ValueError("measures[%d]: %s must be positive and finite" % (k, name))
        arr[k] = m
    return arr


def _round_ends_arg(round_ends, n_rois):
    """(int64 array, count) of the round ends of ife_roi_coverage, with the refusals that need no
    device."""
    ends = [int(v) for v in round_ends]
    if not 1 <= len(ends) <= 64:
        raise ValueError("between 1 and 64 round ends are required (got %d)" % len(ends))
    if any(b < a for a, b in zip([0] + ends, ends)):
        raise ValueError("round_ends must be non-negative and must not decrease")
    if ends[-1] > int(n_rois):
        raise ValueError("round end %d lies beyond the %d boxes" % (ends[-1], int(n_rois)))
    return (C.c_int64 * len(ends))(*ends), len(ends)


def _ptr_array(ptrs):
    return (C.c_void_p * len(ptrs))(*ptrs)


def _order_array(orders):
    """Per-job orders of the recursive Gaussian; None is the C NULL (all zero)."""
    if orders is None:
        return None
    return (C.c_int * len(orders))(*[int(o) for o in orders])


def _double_array(values):
    return (C.c_double * len(values))(*[float(v) for v in values])


class ScaleStream:
    """The scale stream of a context (ife_emphysema_features_begin / _fetch / _fetch_deflated /
    _end) as a context manager: every scale is enqueued on entry and stays on the device until
    exit; fetch and fetch_deflated wait for their scale only."""

    def __init__(self, ctx, image, mask, sigmas, spacing, layout):
        self._ctx, self._layout = ctx, layout
        self._image, self._idt = _image_arg(image)
        self._mask, self._mdt, self._mptr = _mask_arg(mask)
        self._desc = _desc(self._image.shape, spacing)
        self._sig, self.n_scales = _sigma_arg(sigmas), len(sigmas)
        self._open = False

    def __enter__(self):
        c = self._ctx
        c._chk(c._lib.ife_emphysema_features_begin(
            c._h, self._image.ctypes.data, self._idt, self._mptr, self._mdt, C.byref(self._desc),
            self._sig, self.n_scales, self._layout))
        self._open = True
        return self

    def __exit__(self, *a):
        if self._open:
            self._open = False
            self._ctx._chk(self._ctx._lib.ife_emphysema_features_end(self._ctx._h))

    def fetch(self, scale):
        shp = self._image.shape
        out = np.empty(shp + (8,) if self._layout == INTERLEAVED else (8,) + shp, np.float32)
        self._ctx._chk(self._ctx._lib.ife_emphysema_features_fetch(self._ctx._h, int(scale), out.ctypes.data))
        return out

    def fetch_deflated(self, scale, component):
        """(DEFLATE blocks, CRC-32) of one component plane of a planar stream."""
        c = self._ctx
        cap = c.deflate_bound(self._image.size * 4)
        out = np.empty(cap, np.uint8)
        n, crc = C.c_size_t(), C.c_uint32()
        c._chk(c._lib.ife_emphysema_features_fetch_deflated(
            c._h, int(scale), int(component), out.ctypes.data, cap, C.byref(n), C.byref(crc)))
        return out[:n.value].tobytes(), int(crc.value)


class Context:
    """One ``ife_ctx``: a device, a stream, a workspace.  Single-owner."""

    def __init__(self, device=0):
        self._lib = load_library()
        h = C.c_void_p()
        rc = self._lib.ife_ctx_create(int(device), C.byref(h))
        if rc != OK:
            raise IfeError(rc, self._lib.ife_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ife_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise IfeError(rc, self._lib.ife_last_error(self._h).decode())
        return rc

    # ---- configuration -----------------------------------------------------
    def set_stream(self, stream_handle):
        self._chk(self._lib.ife_ctx_set_stream(self._h, C.c_void_p(stream_handle or 0)))

    def set_option(self, option, value):
        self._chk(self._lib.ife_ctx_set_option(self._h, int(option), int(value)))

    def reserve(self, shape_zyx, spacing_xyz=(1.0, 1.0, 1.0)):
        d = _desc(shape_zyx, spacing_xyz)
        self._chk(self._lib.ife_ctx_reserve(self._h, C.byref(d)))

    def synchronize(self):
        self._chk(self._lib.ife_ctx_synchronize(self._h))

    def kernel_times(self):
        arr = (KernelTime * MAX_KERNEL_KINDS)()
        n = self._chk(self._lib.ife_get_kernel_times(self._h, arr, MAX_KERNEL_KINDS))
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms))
                for i in range(n)}

    def measure_stream(self, mode, dst_ptr, src_ptr, nbytes, reps=5):
        """GB/s of a 16-byte-per-lane fill (mode 0: bytes written) or copy (mode 1: bytes read +
        written) over device buffers (ife_measure_stream)."""
        ms = C.c_double()
        self._chk(self._lib.ife_measure_stream(self._h, int(mode), C.c_void_p(dst_ptr),
                                               C.c_void_p(src_ptr or 0), C.c_size_t(nbytes),
                                               int(reps), C.byref(ms)))
        return (1 if mode == 0 else 2) * nbytes / (ms.value * 1e-3) / 1e9

    def reset_kernel_times(self):
        self._chk(self._lib.ife_reset_kernel_times(self._h))

    # ---- host-array entry points (numpy in, numpy out) -----------------------
    def eigenvalues(self, A6):
        A6 = np.ascontiguousarray(A6, np.float32)
        n = A6.size // 6
        out = np.empty(A6.shape[:-1] + (3,), np.float32)
        self._chk(self._lib.ife_eigenvalues(self._h, A6.ctypes.data, n, out.ctypes.data, MEM_HOST))
        return out

    def eigenvalue_features(self, A6):
        A6 = np.ascontiguousarray(A6, np.float32)
        n = A6.size // 6
        out = np.empty(A6.shape[:-1] + (6,), np.float32)
        self._chk(self._lib.ife_eigenvalue_features(self._h, A6.ctypes.data, n, out.ctypes.data,
                                                    MEM_HOST))
        return out

    def hessian3d(self, image, spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        image = np.ascontiguousarray(image, np.float32)
        d = _desc(image.shape, spacing)
        out = np.empty(image.shape + (6,) if layout == INTERLEAVED else (6,) + image.shape,
                       np.float32)
        self._chk(self._lib.ife_hessian3d(self._h, image.ctypes.data, C.byref(d), out.ctypes.data,
                                          layout, MEM_HOST))
        return out

    def gradient_magnitude(self, image, spacing=(1.0, 1.0, 1.0)):
        image = np.ascontiguousarray(image, np.float32)
        d = _desc(image.shape, spacing)
        out = np.empty_like(image)
        self._chk(self._lib.ife_gradient_magnitude(self._h, image.ctypes.data, C.byref(d),
                                                   out.ctypes.data, MEM_HOST))
        return out

    def normalized_gaussian_convolution(self, image, certainty, sigma, spacing=(1.0, 1.0, 1.0)):
        image = np.ascontiguousarray(image, np.float32)
        certainty = np.ascontiguousarray(certainty, np.float32)
        d = _desc(image.shape, spacing)
        out = np.empty_like(image)
        self._chk(self._lib.ife_normalized_gaussian_convolution(
            self._h, image.ctypes.data, certainty.ctypes.data, C.byref(d), float(sigma),
            out.ctypes.data, MEM_HOST))
        return out

    def differential_normalized_convolution(self, image, certainty, sigma, axis_xyz,
                                            spacing=(1.0, 1.0, 1.0)):
        image = np.ascontiguousarray(image, np.float32)
        certainty = np.ascontiguousarray(certainty, np.float32)
        d = _desc(image.shape, spacing)
        out = np.empty_like(image)
        self._chk(self._lib.ife_differential_normalized_convolution(
            self._h, image.ctypes.data, certainty.ctypes.data, C.byref(d), float(sigma),
            int(axis_xyz), out.ctypes.data, MEM_HOST))
        return out

    def emphysema_features(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0),
                           layout=INTERLEAVED):
        """One 8-component volume per sigma: shape (S, nz, ny, nx, 8) or (S, 8, nz, ny, nx)."""
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        shp = image.shape + (8,) if layout == INTERLEAVED else (8,) + image.shape
        out = np.empty((len(sigmas),) + shp, np.float32)
        self._chk(self._lib.ife_emphysema_features(
            self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig,
            len(sigmas), out.ctypes.data, layout, MEM_HOST))
        return out

    def normalized_convolution_jet(self, image, certainty, sigma, spacing=(1.0, 1.0, 1.0),
                                   layout=INTERLEAVED):
        """U = {a*cT}/{a*c} with its gradient and Hessian by the quotient rule: (nz, ny, nx, 10) or
        (10, nz, ny, nx), components U, g_x, g_y, g_z, h_xx, h_xy, h_xz, h_yy, h_yz, h_zz."""
        image = np.ascontiguousarray(image, np.float32)
        certainty = np.ascontiguousarray(certainty, np.float32)
        d = _desc(image.shape, spacing)
        out = np.empty(image.shape + (10,) if layout == INTERLEAVED else (10,) + image.shape,
                       np.float32)
        self._chk(self._lib.ife_normalized_convolution_jet(
            self._h, image.ctypes.data, certainty.ctypes.data, C.byref(d), float(sigma),
            out.ctypes.data, layout, MEM_HOST))
        return out

    def differential_features(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0),
                              layout=INTERLEAVED):
        """emphysema_features with gradient and Hessian from the differential normalized
        convolution: shape (S, nz, ny, nx, 8) or (S, 8, nz, ny, nx)."""
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        shp = image.shape + (8,) if layout == INTERLEAVED else (8,) + image.shape
        out = np.empty((len(sigmas),) + shp, np.float32)
        self._chk(self._lib.ife_differential_features(
            self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig,
            len(sigmas), out.ctypes.data, layout, MEM_HOST))
        return out

    def emphysema_features_stream(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0),
                                  layout=INTERLEAVED):
        """Generator over the scales: begin once, yield one 8-component volume per sigma."""
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        self._chk(self._lib.ife_emphysema_features_begin(
            self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig,
            len(sigmas), layout))
        try:
            shp = image.shape + (8,) if layout == INTERLEAVED else (8,) + image.shape
            for k in range(len(sigmas)):
                out = np.empty(shp, np.float32)
                self._chk(self._lib.ife_emphysema_features_fetch(self._h, k, out.ctypes.data))
                yield out
        finally:
            self._chk(self._lib.ife_emphysema_features_end(self._h))

    def scale_stream(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0), layout=PLANAR):
        """The scale stream as an object: ``with ctx.scale_stream(...) as st``, then
        st.fetch(scale) -> (8, nz, ny, nx) and, on a planar stream, st.fetch_deflated(scale,
        component) -> (DEFLATE blocks, CRC-32 of the plane), in any order, until the block is
        left."""
        return ScaleStream(self, image, mask, sigmas, spacing, layout)

    # ---- DEFLATE blocks formed on the device --------------------------------
    def deflate_bound(self, nbytes):
        return int(self._lib.ife_deflate_bound(int(nbytes)))

    def deflate(self, array):
        """(blocks, crc) of the bytes of `array`: complete non-final DEFLATE blocks (a raw stream
        with 03 00 appended) and the CRC-32 of the input (ife_deflate)."""
        a = np.ascontiguousarray(array)
        cap = self.deflate_bound(a.nbytes)
        out = np.empty(max(cap, 1), np.uint8)
        src = a if a.nbytes else np.zeros(1, np.uint8)
        n, crc = C.c_size_t(), C.c_uint32()
        self._chk(self._lib.ife_deflate(self._h, src.ctypes.data, a.nbytes, out.ctypes.data, cap,
                                        C.byref(n), C.byref(crc), MEM_HOST))
        return out[:n.value].tobytes(), int(crc.value)

    def deflate_device(self, ptr, nbytes, out_ptr, capacity):
        """ife_deflate over device pointers of any byte alignment: (bytes written, crc).  IfeError
        E_SIZE when `capacity` is too small; nothing is written then."""
        n, crc = C.c_size_t(), C.c_uint32()
        rc = self._lib.ife_deflate(self._h, C.c_void_p(ptr), int(nbytes), C.c_void_p(out_ptr),
                                   int(capacity), C.byref(n), C.byref(crc), MEM_DEVICE)
        if rc == E_SIZE:
            err = IfeError(rc, self._lib.ife_last_error(self._h).decode())
            err.needed = int(n.value)  # the size the blocks take
            raise err
        self._chk(rc)
        return int(n.value), int(crc.value)

    def fd_hessian_features(self, image, mask=None, spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(image.shape, spacing)
        out = np.empty(image.shape + (6,) if layout == INTERLEAVED else (6,) + image.shape,
                       np.float32)
        self._chk(self._lib.ife_fd_hessian_features(
            self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d),
            out.ctypes.data, layout, MEM_HOST))
        return out

    def fd_gradient_features(self, image, mask_f32=None, spacing=(1.0, 1.0, 1.0)):
        image = np.ascontiguousarray(image, np.float32)
        mptr = None
        if mask_f32 is not None:
            mask_f32 = np.ascontiguousarray(mask_f32, np.float32)
            mptr = mask_f32.ctypes.data
        d = _desc(image.shape, spacing)
        out = np.empty_like(image)
        self._chk(self._lib.ife_fd_gradient_features(self._h, image.ctypes.data, mptr, C.byref(d),
                                                     out.ctypes.data, MEM_HOST))
        return out

    def mask_image_f64(self, image, mask, outside=0.0):
        image = np.ascontiguousarray(image, np.float64)
        mask = np.ascontiguousarray(mask, np.float64)
        out = np.empty_like(image)
        self._chk(self._lib.ife_mask_image_f64(self._h, image.ctypes.data, mask.ctypes.data,
                                               float(outside), image.size, out.ctypes.data,
                                               MEM_HOST))
        return out

    # ---- signed Maurer distance map, expected distance --------------------------
    def signed_distance_map(self, mask, spacing=(1.0, 1.0, 1.0), inside_is_positive=True,
                            squared=False):
        """float64 [z, y, x]: distance to the six-neighbour contour of mask != 0, positive inside
        (or outside); +-sqrt(DBL_MAX) (+-DBL_MAX squared) everywhere when there is no contour."""
        if mask is None:
            raise TypeError("a mask is required")
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(mask.shape, spacing)
        out = np.empty(mask.shape, np.float64)
        self._chk(self._lib.ife_signed_distance_map(
            self._h, mptr, mdt, C.byref(d), int(bool(inside_is_positive)), int(bool(squared)),
            out.ctypes.data, MEM_HOST))
        return out

    def expected_distance(self, mask, prob, spacing=(1.0, 1.0, 1.0)):
        """(mean over mask != 0 of distance map * prob, number of voxels with mask != 0)."""
        if mask is None:
            raise TypeError("a mask is required")
        mask, mdt, mptr = _mask_arg(mask)
        prob = np.ascontiguousarray(prob, np.float64)
        if prob.shape != mask.shape:
            raise ValueError("mask and prob differ in shape")
        d = _desc(mask.shape, spacing)
        value, n = C.c_double(), C.c_int64()
        self._chk(self._lib.ife_expected_distance(
            self._h, mptr, mdt, prob.ctypes.data, C.byref(d), C.byref(value), C.byref(n), MEM_HOST))
        return value.value, n.value

    # ---- resampling onto a target grid ---------------------------------------------
    def _resample(self, src_ptr, src_dtype, src_shape, src_spacing, src_origin, dst_shape, dst_spacing,
                  dst_origin, translation, interpolation, default, out_ptr, mem):
        sd, dd = _desc(src_shape, src_spacing), _desc(dst_shape, dst_spacing)
        geom = (C.byref(sd), _double_array(src_origin), C.byref(dd), _double_array(dst_origin),
                _double_array(translation), int(interpolation), float(default), C.c_void_p(out_ptr or 0), mem)
        if src_dtype is None:
            self._chk(self._lib.ife_resample_f64(self._h, C.c_void_p(src_ptr or 0), *geom))
        else:
            self._chk(self._lib.ife_resample(self._h, C.c_void_p(src_ptr or 0), int(src_dtype), *geom))

    def resample(self, src, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin,
                 translation=(0, 0, 0), interpolation=INTERP_LINEAR, default=0.0):
        """src [z, y, x] on the grid (dst_shape (nz, ny, nx), dst_spacing, dst_origin); spacings,
        origins and the translation are (x, y, z).  float64 in gives float64 out; float32, int16,
        uint8 and uint16 give float32 (linear) or their own dtype (nearest)."""
        src = np.ascontiguousarray(src)
        if src.ndim != 3:
            raise ValueError("src must have three dimensions")
        if src.dtype == np.float64:
            dt, odt = None, np.float64
        elif src.dtype in _RESAMPLE_DT:
            dt = _RESAMPLE_DT[src.dtype]
            odt = np.float32 if interpolation == INTERP_LINEAR else src.dtype
        else:
            raise TypeError("src must be float64, float32, int16, uint8 or uint16")
        out = np.empty(tuple(int(v) for v in dst_shape), odt)
        self._resample(src.ctypes.data, dt, src.shape, src_spacing, src_origin, out.shape, dst_spacing,
                       dst_origin, translation, interpolation, default, out.ctypes.data, MEM_HOST)
        return out

    def resample_device(self, src_ptr, src_dtype, src_shape, src_spacing, src_origin, dst_shape,
                        dst_spacing, dst_origin, out_ptr, translation=(0, 0, 0),
                        interpolation=INTERP_LINEAR, default=0.0):
        """Enqueues on the context's stream.  src_dtype None: float64 in and out
        (ife_resample_f64); else out_ptr is float32 (linear) or the source's type (nearest)."""
        self._resample(src_ptr, src_dtype, src_shape, src_spacing, src_origin, dst_shape, dst_spacing,
                       dst_origin, translation, interpolation, default, out_ptr, MEM_DEVICE)

    # ---- B-spline resampling (orders 0 to 5) and the 8-bit window -------------------
    @staticmethod
    def _bspline_source(src):
        src = np.ascontiguousarray(src)
        if src.ndim != 3:
            raise ValueError("src must have three dimensions")
        if src.dtype == np.float64:
            return src, None
        if src.dtype not in _RESAMPLE_DT:
            raise TypeError("src must be float64, float32, int16, uint8 or uint16")
        return src, _RESAMPLE_DT[src.dtype]

    def bspline_coefficients_device(self, src_ptr, src_dtype, shape_zyx, order, coef_ptr):
        """Enqueues on the context's stream; coef_ptr: float64 [z, y, x] in device memory.
        src_dtype None: float64 source (ife_bspline_coefficients_f64), where coef_ptr may equal
        src_ptr (in place)."""
        d = _desc(shape_zyx, (1.0, 1.0, 1.0))
        if src_dtype is None:
            self._chk(self._lib.ife_bspline_coefficients_f64(self._h, C.c_void_p(src_ptr or 0), C.byref(d),
                                                             int(order), C.c_void_p(coef_ptr or 0), MEM_DEVICE))
        else:
            self._chk(self._lib.ife_bspline_coefficients(self._h, C.c_void_p(src_ptr or 0), int(src_dtype),
                                                         C.byref(d), int(order), C.c_void_p(coef_ptr or 0),
                                                         MEM_DEVICE))

    def bspline_coefficients(self, src, order=3):
        """The B-spline coefficients of src [z, y, x] (float64, float32, int16, uint8 or uint16)
        for `order` in 0..5, as float64 (include/ife_hip.h states the arithmetic)."""
        src, dt = self._bspline_source(src)
        coef = np.empty(src.shape, np.float64)
        d = _desc(src.shape, (1.0, 1.0, 1.0))
        if dt is None:
            self._chk(self._lib.ife_bspline_coefficients_f64(self._h, src.ctypes.data, C.byref(d), int(order),
                                                             coef.ctypes.data, MEM_HOST))
        else:
            self._chk(self._lib.ife_bspline_coefficients(self._h, src.ctypes.data, dt, C.byref(d), int(order),
                                                         coef.ctypes.data, MEM_HOST))
        return coef

    def _resample_bspline(self, src_ptr, src_dtype, src_shape, src_spacing, src_origin, dst_shape, dst_spacing,
                          dst_origin, translation, order, extrapolate, default, out_ptr, mem):
        sd, dd = _desc(src_shape, src_spacing), _desc(dst_shape, dst_spacing)
        geom = (C.byref(sd), _double_array(src_origin), C.byref(dd), _double_array(dst_origin),
                _double_array(translation), int(order), int(extrapolate), float(default),
                C.c_void_p(out_ptr or 0), mem)
        if src_dtype is None:
            self._chk(self._lib.ife_resample_bspline_f64(self._h, C.c_void_p(src_ptr or 0), *geom))
        else:
            self._chk(self._lib.ife_resample_bspline(self._h, C.c_void_p(src_ptr or 0), int(src_dtype), *geom))

    def resample_bspline(self, src, src_spacing, src_origin, dst_shape, dst_spacing, dst_origin,
                         translation=(0, 0, 0), order=3, extrapolate=False, default=0.0):
        """src [z, y, x] on the grid (dst_shape (nz, ny, nx), dst_spacing, dst_origin) through a
        B-spline of `order` 0..5; spacings, origins and the translation are (x, y, z).  Outside
        voxels get `default`, or with extrapolate the nearest source voxel.  float64 in gives
        float64 out; float32, int16, uint8 and uint16 give float32."""
        src, dt = self._bspline_source(src)
        out = np.empty(tuple(int(v) for v in dst_shape), np.float64 if dt is None else np.float32)
        self._resample_bspline(src.ctypes.data, dt, src.shape, src_spacing, src_origin, out.shape, dst_spacing,
                               dst_origin, translation, order, extrapolate, default, out.ctypes.data, MEM_HOST)
        return out

    def resample_bspline_device(self, src_ptr, src_dtype, src_shape, src_spacing, src_origin, dst_shape,
                                dst_spacing, dst_origin, out_ptr, translation=(0, 0, 0), order=3,
                                extrapolate=False, default=0.0):
        """Enqueues on the context's stream.  src_dtype None: float64 in and out
        (ife_resample_bspline_f64); else out_ptr is float32."""
        self._resample_bspline(src_ptr, src_dtype, src_shape, src_spacing, src_origin, dst_shape, dst_spacing,
                               dst_origin, translation, order, extrapolate, default, out_ptr, MEM_DEVICE)

    def window_u8_device(self, src_ptr, mask_ptr, n, window_min, window_max, out_ptr, out_min=0, out_max=255):
        """Enqueues on the context's stream; src_ptr and mask_ptr (0: no mask): n float64,
        out_ptr: n uint8, all in device memory."""
        self._chk(self._lib.ife_window_u8(self._h, C.c_void_p(src_ptr or 0), C.c_void_p(mask_ptr or 0), int(n),
                                          float(window_min), float(window_max), int(out_min), int(out_max),
                                          C.c_void_p(out_ptr or 0), MEM_DEVICE))

    def window_u8(self, src, window_min, window_max, mask=None, out_min=0, out_max=255):
        """float64 values windowed to uint8: below window_min out_min, above window_max out_max,
        linear between (truncated); where a float64 mask of the same shape is 0 the result is 0."""
        src = np.ascontiguousarray(src, np.float64)
        if mask is not None:
            mask = np.ascontiguousarray(mask, np.float64)
            if mask.shape != src.shape:
                raise ValueError("mask and src differ in shape")
        out = np.empty(src.shape, np.uint8)
        self._chk(self._lib.ife_window_u8(self._h, src.ctypes.data, None if mask is None else mask.ctypes.data,
                                          src.size, float(window_min), float(window_max), int(out_min),
                                          int(out_max), out.ctypes.data, MEM_HOST))
        return out

    # ---- device-pointer entry points (inputs already in HBM) ------------------
    def signed_distance_map_device(self, mask_ptr, mask_dtype, shape_zyx, spacing, out_ptr,
                                   inside_is_positive=True, squared=False):
        """Enqueues on the context's stream; out_ptr: float64 [z, y, x] in device memory."""
        d = _desc(shape_zyx, spacing)
        self._chk(self._lib.ife_signed_distance_map(
            self._h, C.c_void_p(mask_ptr or 0), mask_dtype, C.byref(d),
            int(bool(inside_is_positive)), int(bool(squared)), C.c_void_p(out_ptr or 0), MEM_DEVICE))

    def emphysema_features_device(self, image_ptr, image_dtype, mask_ptr, mask_dtype, shape_zyx,
                                  spacing, sigmas, out_ptr, layout=INTERLEAVED):
        d = _desc(shape_zyx, spacing)
        sig = _sigma_arg(sigmas)
        self._chk(self._lib.ife_emphysema_features(
            self._h, C.c_void_p(image_ptr), image_dtype, C.c_void_p(mask_ptr or 0), mask_dtype,
            C.byref(d), sig, len(sigmas), C.c_void_p(out_ptr), layout, MEM_DEVICE))

    def differential_features_device(self, image_ptr, image_dtype, mask_ptr, mask_dtype, shape_zyx,
                                     spacing, sigmas, out_ptr, layout=INTERLEAVED):
        d = _desc(shape_zyx, spacing)
        sig = _sigma_arg(sigmas)
        self._chk(self._lib.ife_differential_features(
            self._h, C.c_void_p(image_ptr), image_dtype, C.c_void_p(mask_ptr or 0), mask_dtype,
            C.byref(d), sig, len(sigmas), C.c_void_p(out_ptr), layout, MEM_DEVICE))

    def normalized_convolution_jet_device(self, image_ptr, certainty_ptr, shape_zyx, spacing, sigma,
                                          out_ptr, layout=INTERLEAVED):
        d = _desc(shape_zyx, spacing)
        self._chk(self._lib.ife_normalized_convolution_jet(
            self._h, C.c_void_p(image_ptr), C.c_void_p(certainty_ptr), C.byref(d), float(sigma),
            C.c_void_p(out_ptr), layout, MEM_DEVICE))

    def fd_hessian_features_device(self, image_ptr, image_dtype, mask_ptr, mask_dtype, shape_zyx,
                                   spacing, out_ptr, layout=INTERLEAVED):
        d = _desc(shape_zyx, spacing)
        self._chk(self._lib.ife_fd_hessian_features(
            self._h, C.c_void_p(image_ptr), image_dtype, C.c_void_p(mask_ptr or 0), mask_dtype,
            C.byref(d), C.c_void_p(out_ptr), layout, MEM_DEVICE))

    # ---- stage entry points (device pointers; Z-slab orchestration, slab.py) ------------
    def stage_prepare(self, image_ptr, image_dtype, mask_ptr, mask_dtype, slab_shape_zyx, tc_ptr,
                      cf_ptr, y_chunks=1):
        d = _desc(slab_shape_zyx, (1.0, 1.0, 1.0))
        self._chk(self._lib.ife_stage_prepare(
            self._h, C.c_void_p(image_ptr), image_dtype, C.c_void_p(mask_ptr or 0), mask_dtype,
            C.byref(d), int(y_chunks), C.c_void_p(tc_ptr), C.c_void_p(cf_ptr or 0)))

    def stage_recursive_gaussian(self, in_ptr, out_ptr, shape_zyx, spacing, axis_xyz, sigma):
        d = _desc(shape_zyx, spacing)
        self._chk(self._lib.ife_stage_recursive_gaussian(
            self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.byref(d), int(axis_xyz),
            float(sigma)))

    def stage_recursive_gaussian_order(self, in_ptr, out_ptr, shape_zyx, spacing, axis_xyz, sigma,
                                       order):
        """One axis pass of ITK's recursive Gaussian of order 0, 1 or 2 (pixel units)."""
        d = _desc(shape_zyx, spacing)
        self._chk(self._lib.ife_stage_recursive_gaussian_order(
            self._h, C.c_void_p(in_ptr), C.c_void_p(out_ptr), C.byref(d), int(axis_xyz),
            float(sigma), int(order)))

    def stage_recursive_gaussian_batch(self, in_ptrs, out_ptrs, shape_zyx, spacing, axis_xyz,
                                       sigmas, in_y_chunks=1):
        """One launch over len(in_ptrs) float volumes of the same shape (<= 8 jobs)."""
        d = _desc(shape_zyx, spacing)
        self._chk(self._lib.ife_stage_recursive_gaussian_batch(
            self._h, len(in_ptrs), _ptr_array(in_ptrs), _ptr_array(out_ptrs), C.byref(d), int(axis_xyz),
            _double_array(sigmas), int(in_y_chunks)))

    def stage_features(self, num_ptr, den_ptr, mask_ptr, mask_dtype, slab_shape_zyx, spacing,
                       halo_lo, halo_hi, out_ptr, layout=INTERLEAVED):
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_features(
            self._h, C.c_void_p(num_ptr), C.c_void_p(den_ptr or 0), C.c_void_p(mask_ptr or 0),
            mask_dtype, C.byref(d), int(bool(halo_lo)), int(bool(halo_hi)), C.c_void_p(out_ptr),
            layout))

    def stage_z_ck_bytes(self, slab_shape_zyx):
        d = _desc(slab_shape_zyx, (1.0, 1.0, 1.0))
        return int(self._lib.ife_stage_z_ck_bytes(C.byref(d)))

    def stage_z_sweep(self, direction, in_ptrs, slab_shape_zyx, spacing, line0, nlines, sigmas,
                      has_neighbour, state_in_ptr, state_out_ptr, ck_ptrs):
        """Causal (direction 0) or anticausal (1) sweep of the Z pass of a Z-slab."""
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_z_sweep(
            self._h, int(direction), len(in_ptrs), _ptr_array(in_ptrs), C.byref(d), int(line0), int(nlines),
            _double_array(sigmas), int(bool(has_neighbour)), C.c_void_p(state_in_ptr or 0),
            C.c_void_p(state_out_ptr), _ptr_array(ck_ptrs)))

    def stage_z_combine(self, in_ptrs, out_ptrs, slab_shape_zyx, spacing, line0, nlines, sigmas,
                        has_lo, has_hi, ck_ptrs):
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_z_combine(
            self._h, len(in_ptrs), _ptr_array(in_ptrs), _ptr_array(out_ptrs), C.byref(d), int(line0),
            int(nlines), _double_array(sigmas), int(bool(has_lo)), int(bool(has_hi)), _ptr_array(ck_ptrs)))

    def stage_z_fused(self, direction, in_ptrs, out_ptrs, slab_shape_zyx, spacing, line0, nlines,
                      sigmas, has_lo, has_hi, state_in_ptr, state_out_ptr, ck_ptrs):
        """Sweep of `direction` (0 causal, 1 anticausal) and combine in one launch."""
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_z_fused(
            self._h, int(direction), len(in_ptrs), _ptr_array(in_ptrs), _ptr_array(out_ptrs), C.byref(d),
            int(line0), int(nlines), _double_array(sigmas), int(bool(has_lo)), int(bool(has_hi)),
            C.c_void_p(state_in_ptr or 0), C.c_void_p(state_out_ptr), _ptr_array(ck_ptrs)))

    def stage_z_sweep_order(self, direction, in_ptrs, slab_shape_zyx, spacing, line0, nlines, sigmas,
                            orders, has_neighbour, state_in_ptr, state_out_ptr, ck_ptrs):
        """stage_z_sweep with an order (0, 1, 2) per job; orders None = all zero.  Three
        consecutive jobs with the same input, the same sigma and the orders 0, 1, 2 read every
        plane once."""
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_z_sweep_order(
            self._h, int(direction), len(in_ptrs), _ptr_array(in_ptrs), C.byref(d), int(line0), int(nlines),
            _double_array(sigmas), _order_array(orders), int(bool(has_neighbour)),
            C.c_void_p(state_in_ptr or 0), C.c_void_p(state_out_ptr), _ptr_array(ck_ptrs)))

    def stage_z_combine_order(self, in_ptrs, out_ptrs, slab_shape_zyx, spacing, line0, nlines, sigmas,
                              orders, has_lo, has_hi, ck_ptrs):
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_z_combine_order(
            self._h, len(in_ptrs), _ptr_array(in_ptrs), _ptr_array(out_ptrs), C.byref(d), int(line0),
            int(nlines), _double_array(sigmas), _order_array(orders), int(bool(has_lo)), int(bool(has_hi)),
            _ptr_array(ck_ptrs)))

    def stage_z_fused_order(self, direction, in_ptrs, out_ptrs, slab_shape_zyx, spacing, line0, nlines,
                            sigmas, orders, has_lo, has_hi, state_in_ptr, state_out_ptr, ck_ptrs):
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_z_fused_order(
            self._h, int(direction), len(in_ptrs), _ptr_array(in_ptrs), _ptr_array(out_ptrs), C.byref(d),
            int(line0), int(nlines), _double_array(sigmas), _order_array(orders), int(bool(has_lo)),
            int(bool(has_hi)), C.c_void_p(state_in_ptr or 0), C.c_void_p(state_out_ptr), _ptr_array(ck_ptrs)))

    def stage_jet_features(self, zf_ptrs, mask_ptr, mask_dtype, slab_shape_zyx, spacing, sigma, out_ptr,
                           layout=INTERLEAVED):
        """X level, Y level and pointwise pass of differential_features on a slab, from its six
        Z-level fields: zf_ptrs[3 * s + k] = source s (0 cT, 1 c) at order k."""
        if len(zf_ptrs) != 6:
            raise ValueError("six Z-level fields are required")
        d = _desc(slab_shape_zyx, spacing)
        self._chk(self._lib.ife_stage_jet_features(
            self._h, _ptr_array(zf_ptrs), C.c_void_p(mask_ptr or 0), mask_dtype, C.byref(d), float(sigma),
            C.c_void_p(out_ptr), layout))

    def stage_recursive_gaussian_quotient(self, num_ptrs, den_ptrs, out_ptrs, shape_zyx, spacing,
                                          axis_xyz, sigmas):
        """Last axis pass in its quotient form: out[j] = G(num[j]) / G(den[j]) (<= 4 jobs)."""
        d = _desc(shape_zyx, spacing)
        self._chk(self._lib.ife_stage_recursive_gaussian_quotient(
            self._h, len(num_ptrs), _ptr_array(num_ptrs), _ptr_array(den_ptrs), _ptr_array(out_ptrs),
            C.byref(d), int(axis_xyz), _double_array(sigmas)))

    # ---- rows f1 / f2: sample columns, histogram edges, dense histograms --------------
    def sort_f32(self, values):
        v = np.ascontiguousarray(values, np.float32).ravel()
        out = np.empty_like(v)
        self._chk(self._lib.ife_sort_f32(self._h, v.ctypes.data, v.size, out.ctypes.data, MEM_HOST))
        return out

    def sort_f32_device(self, in_ptr, n, out_ptr):
        self._chk(self._lib.ife_sort_f32(self._h, C.c_void_p(in_ptr), int(n), C.c_void_p(out_ptr),
                                         MEM_DEVICE))

    def equalized_edges(self, sorted_values, nbins):
        """determineEdgesForEqualizedHistogram on an ascending float32 (or float64) array."""
        v = np.ascontiguousarray(sorted_values)
        if v.dtype == np.float64:
            out = np.empty(max(int(nbins) - 1, 0), np.float64)
            self._chk(self._lib.ife_equalized_edges_f64(self._h, v.ctypes.data, v.size, int(nbins),
                                                        out.ctypes.data, MEM_HOST))
            return out
        v = np.ascontiguousarray(v, np.float32).ravel()
        out = np.empty(max(int(nbins) - 1, 0), np.float32)
        self._chk(self._lib.ife_equalized_edges_f32(self._h, v.ctypes.data, v.size, int(nbins),
                                                    out.ctypes.data, MEM_HOST))
        return out

    def dense_histogram(self, edges, values):
        e = np.ascontiguousarray(edges, np.float32).ravel()
        v = np.ascontiguousarray(values, np.float32).ravel()
        counts = np.empty(e.size + 1, np.uint32)
        self._chk(self._lib.ife_dense_histogram_f32(self._h, e.ctypes.data, e.size, v.ctypes.data,
                                                    v.size, counts.ctypes.data, MEM_HOST))
        return counts

    def roi_histograms(self, features, mask, rois, edges, spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        """Bag rows of one feature volume: counts (n_rois, ncomp, n_edges+1) uint32."""
        f = np.ascontiguousarray(features, np.float32)
        mask, mdt, mptr = _mask_arg(mask)
        rois = np.ascontiguousarray(rois, np.int64).reshape(-1, 6)
        edges = np.ascontiguousarray(edges, np.float32)
        ncomp, ne = edges.shape
        d = _desc(mask.shape, spacing)
        counts = np.empty((rois.shape[0], ncomp, ne + 1), np.uint32)
        self._chk(self._lib.ife_roi_histograms(
            self._h, f.ctypes.data, layout, ncomp, mptr, mdt, C.byref(d),
            rois.ctypes.data, rois.shape[0], edges.ctypes.data, ne, counts.ctypes.data, MEM_HOST))
        return counts

    def bag_image(self, image, mask, sigmas, rois, edges, spacing=(1.0, 1.0, 1.0)):
        """One image of MakeBag: counts (n_rois, n_sigmas*8, n_edges+1) uint32."""
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        rois = np.ascontiguousarray(rois, np.int64).reshape(-1, 6)
        edges = np.ascontiguousarray(edges, np.float32)
        ne = edges.shape[1]
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        counts = np.empty((rois.shape[0], 8 * len(sigmas), ne + 1), np.uint32)
        self._chk(self._lib.ife_bag_image(
            self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig, len(sigmas), rois.ctypes.data,
            rois.shape[0], edges.ctypes.data, ne,
            counts.ctypes.data, MEM_HOST))
        return counts

    # ---- the dense bag: one region per mask voxel whose box fits ----------------------
    def _dense_count(self, gen_mask, size_xyz, spacing=(1.0, 1.0, 1.0)):
        """Number of regions of DenseROIGenerator(gen_mask).generate(size)."""
        gen_mask, gdt, gptr = _mask_arg(gen_mask)
        d = _desc(gen_mask.shape, spacing)
        n = C.c_int64()
        self._chk(self._lib.ife_dense_rois(self._h, gptr, gdt, C.byref(d), _size_arg(size_xyz),
                                           C.byref(n), None, 0, MEM_HOST))
        return n.value

    def dense_rois(self, mask, size):
        """Boxes (n, 6) int64 {x0, y0, z0, sx, sy, sz} around every voxel of mask != 0 whose box
        of `size` = (sx, sy, sz) fits the volume, raster order."""
        if mask is None:
            raise TypeError("a mask is required")
        n = self._dense_count(mask, size)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(mask.shape, (1.0, 1.0, 1.0))
        rois = np.empty((max(n, 1), 6), np.int64)
        got = C.c_int64()
        self._chk(self._lib.ife_dense_rois(self._h, mptr, mdt, C.byref(d), _size_arg(size),
                                           C.byref(got), rois.ctypes.data, rois.shape[0], MEM_HOST))
        return rois[:got.value]

    def dense_roi_histograms(self, features, mask, size, edges, gen_mask=None,
                             spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        """ctx.roi_histograms for the boxes of ctx.dense_rois(gen_mask or mask, size), without the
        boxes: counts (n_rois, ncomp, n_edges+1) uint32."""
        if mask is None:
            raise TypeError("a mask is required")
        f = np.ascontiguousarray(features, np.float32)
        n = self._dense_count(mask if gen_mask is None else gen_mask, size, spacing)
        mask, mdt, mptr = _mask_arg(mask)
        gen_mask, gdt, gptr = _mask_arg(gen_mask)
        edges = np.ascontiguousarray(edges, np.float32)
        ncomp, ne = edges.shape
        d = _desc(mask.shape, spacing)
        counts = np.empty((max(n, 1), ncomp, ne + 1), np.uint32)
        got = C.c_int64()
        self._chk(self._lib.ife_dense_roi_histograms(
            self._h, f.ctypes.data, layout, ncomp, mptr, mdt, gptr, gdt, C.byref(d), _size_arg(size),
            edges.ctypes.data, ne, counts.ctypes.data, counts.shape[0], C.byref(got), MEM_HOST))
        return counts[:got.value]

    def bag_image_dense(self, image, mask, sigmas, size, edges, gen_mask=None,
                        spacing=(1.0, 1.0, 1.0)):
        """One image of MakeBagDense: counts (n_rois, n_sigmas*8, n_edges+1) uint32."""
        if mask is None:
            raise TypeError("a mask is required")
        image, idt = _image_arg(image)
        n = self._dense_count(mask if gen_mask is None else gen_mask, size, spacing)
        mask, mdt, mptr = _mask_arg(mask)
        gen_mask, gdt, gptr = _mask_arg(gen_mask)
        edges = np.ascontiguousarray(edges, np.float32)
        ne = edges.shape[1]
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        counts = np.empty((max(n, 1), 8 * len(sigmas), ne + 1), np.uint32)
        got = C.c_int64()
        self._chk(self._lib.ife_bag_image_dense(
            self._h, image.ctypes.data, idt, mptr, mdt, gptr, gdt, C.byref(d), sig, len(sigmas),
            _size_arg(size), edges.ctypes.data, ne, counts.ctypes.data, counts.shape[0],
            C.byref(got), MEM_HOST))
        return counts[:got.value]

    # ---- per-region label modes (ExtractLabels) ----------------------------------------
    def roi_labels(self, labels, rois, ignore=(), dominant=-1):
        """The mode of the uint8 label volume inside every box of rois (n, 6) {x, y, z, sx, sy,
        sz}: (n,) uint8.  ignore: labels that do not vote; dominant: a label that wins wherever
        it occurs (-1: none); ties go to the smallest label (include/ife_hip.h has the rule)."""
        labels = _labels_arg(labels)
        rois = np.ascontiguousarray(rois, np.int64).reshape(-1, 6)
        ign, n_ign = _ignore_arg(ignore)
        d = _desc(labels.shape, (1.0, 1.0, 1.0))
        out = np.empty(rois.shape[0], np.uint8)
        self._chk(self._lib.ife_roi_labels(self._h, labels.ctypes.data, U8, C.byref(d), rois.ctypes.data,
                                           rois.shape[0], ign, n_ign, int(dominant), out.ctypes.data, MEM_HOST))
        return out

    def dense_roi_labels(self, labels, gen_mask, size, ignore=(), dominant=-1):
        """ctx.roi_labels for the boxes of ctx.dense_rois(gen_mask, size), without the boxes: the
        labels of a dense bag in the row order of the bag, (n_rois,) uint8."""
        if gen_mask is None:
            raise TypeError("a generating mask is required")
        labels = _labels_arg(labels)
        n = self._dense_count(gen_mask, size)
        gen_mask, gdt, gptr = _mask_arg(gen_mask)
        if gen_mask.shape != labels.shape:
            raise ValueError("labels and gen_mask differ in shape")
        ign, n_ign = _ignore_arg(ignore)
        d = _desc(labels.shape, (1.0, 1.0, 1.0))
        out = np.empty(max(n, 1), np.uint8)
        got = C.c_int64()
        self._chk(self._lib.ife_dense_roi_labels(
            self._h, labels.ctypes.data, U8, gptr, gdt, C.byref(d), _size_arg(size), ign, n_ign, int(dominant),
            out.ctypes.data, out.shape[0], C.byref(got), MEM_HOST))
        return out[:got.value]

    # ---- regions: mask bounding box, crop / pad / flip, label sets --------------------------
    def mask_bounding_box_device(self, ptr, dtype, shape_zyx):
        """((x0, y0, z0), (sx, sy, sz), count) of the foreground of a device mask of dtype code
        U8, U16, I16 or F32; an empty mask gives zeros."""
        d = _desc(shape_zyx, (1.0, 1.0, 1.0))
        box = (C.c_int64 * 6)()
        count = C.c_int64()
        self._chk(self._lib.ife_mask_bounding_box(self._h, C.c_void_p(ptr or 0), int(dtype), C.byref(d), box,
                                                  C.byref(count), MEM_DEVICE))
        return tuple(box[0:3]), tuple(box[3:6]), count.value

    def mask_bounding_box(self, mask):
        """The tightest box around the foreground of a (z, y, x) mask (uint8, uint16, int16: != 0;
        float32: any bit pattern but +-0) and the number of foreground voxels:
        ((x0, y0, z0), (sx, sy, sz), count); an empty mask gives zeros."""
        mask = np.ascontiguousarray(mask)
        if mask.dtype not in _BOX_DT:
            raise TypeError("mask must be uint8, uint16, int16 or float32")
        if mask.ndim != 3:
            raise ValueError("mask must be a (z, y, x) volume")
        d = _desc(mask.shape, (1.0, 1.0, 1.0))
        box = (C.c_int64 * 6)()
        count = C.c_int64()
        self._chk(self._lib.ife_mask_bounding_box(self._h, mask.ctypes.data, _BOX_DT[mask.dtype], C.byref(d), box,
                                                  C.byref(count), MEM_HOST))
        return tuple(box[0:3]), tuple(box[3:6]), count.value

    def extract_region_device(self, src_ptr, elem_bytes, src_shape_zyx, index_xyz, size_xyz, dst_ptr,
                              pad_value=None, flip=(False, False, False)):
        """Enqueues on the context's stream and waits; src_ptr: the source, dst_ptr: size_xyz
        elements of elem_bytes bytes, both in device memory.  pad_value: None or elem_bytes bytes."""
        region, bits = _region_arg(index_xyz, size_xyz, flip, int(elem_bytes), src_shape_zyx, pad_value is not None)
        pad = None if pad_value is None else bytes(pad_value)
        if pad is not None and len(pad) != int(elem_bytes):
            raise ValueError("pad_value must hold elem_bytes bytes")
        d = _desc(src_shape_zyx, (1.0, 1.0, 1.0))
        self._chk(self._lib.ife_extract_region(self._h, C.c_void_p(src_ptr or 0), int(elem_bytes), C.byref(d), region,
                                               bits, pad, C.c_void_p(dst_ptr or 0), MEM_DEVICE, MEM_DEVICE))

    def extract_region(self, src, index_xyz, size_xyz, pad_value=None, flip=(False, False, False)):
        """The box of size_xyz at index_xyz of a (z, y, x) volume of any dtype of 1, 2, 4 or 8
        bytes, as a new (sz, sy, sx) array of that dtype: a crop where the box is inside, a
        constant pad (pad_value) where it reaches outside, mirrored along the axes of flip
        (x, y, z).  Bits are copied, nothing is converted."""
        src = np.ascontiguousarray(src)
        if src.ndim != 3:
            raise ValueError("src must be a (z, y, x) volume")
        region, bits = _region_arg(index_xyz, size_xyz, flip, src.dtype.itemsize, src.shape, pad_value is not None)
        pad = None if pad_value is None else np.array(pad_value, dtype=src.dtype).tobytes()
        d = _desc(src.shape, (1.0, 1.0, 1.0))
        out = np.empty((region[5], region[4], region[3]), src.dtype)
        self._chk(self._lib.ife_extract_region(self._h, src.ctypes.data, src.dtype.itemsize, C.byref(d), region, bits,
                                               pad, out.ctypes.data, MEM_HOST, MEM_HOST))
        return out

    def label_membership_device(self, labels_ptr, dtype, n, include, out_ptr, inside=1, outside=0):
        """Enqueues on the context's stream and waits; labels_ptr and out_ptr: n elements of dtype
        code U8 or U16 in device memory."""
        if dtype not in (U8, U16):
            raise TypeError("labels must be uint8 or uint16")
        inc, n_inc = _include_arg(include, inside, outside, np.uint8 if dtype == U8 else np.uint16)
        self._chk(self._lib.ife_label_membership(self._h, C.c_void_p(labels_ptr or 0), dtype, int(n), inc, n_inc,
                                                 int(inside), int(outside), C.c_void_p(out_ptr or 0), MEM_DEVICE))

    def label_membership(self, labels, include, inside=1, outside=0):
        """`inside` where a uint8 or uint16 label occurs in `include`, `outside` elsewhere; the
        result has the labels' shape and dtype.  include needs no order and may repeat values."""
        labels = np.ascontiguousarray(labels)
        if labels.dtype not in _MSK_DT:
            raise TypeError("labels must be uint8 or uint16")
        inc, n_inc = _include_arg(include, inside, outside, labels.dtype)
        out = np.empty(labels.shape, labels.dtype)
        if labels.size:
            self._chk(self._lib.ife_label_membership(self._h, labels.ctypes.data, _MSK_DT[labels.dtype], labels.size,
                                                     inc, n_inc, int(inside), int(outside), out.ctypes.data,
                                                     MEM_HOST))
        return out

    # ---- sampling: seeded draws of mask voxels and boxes, a batched box gather --------------
    def _draw(self, name, mask_ptr, dtype, shape_zyx, out_ptr, mem, args, n_sets):
        """One of the two sampling calls; returns n_admissible (n_sets,) int64.  Where a set is
        empty and draws were asked for, the IfeError carries the counts as .n_admissible."""
        d = _desc(shape_zyx, (1.0, 1.0, 1.0))
        counts = np.zeros(n_sets, np.int64)
        try:
            self._chk(getattr(self._lib, name)(self._h, C.c_void_p(mask_ptr or 0), int(dtype), C.byref(d), *args,
                                               C.c_void_p(out_ptr or 0),
                                               counts.ctypes.data_as(C.POINTER(C.c_int64)), mem))
        except IfeError as e:
            e.n_admissible = counts
            raise
        return counts

    def sample_positions_device(self, mask_ptr, dtype, shape_zyx, out_ptr, n_draws, size=(1, 1, 1), values=(),
                                per_value=False, seed=0, stream=0, first_draw=0):
        """Enqueues on the context's stream and waits; mask_ptr: the mask of dtype code U8 or U16,
        out_ptr: sets * n_draws int64, both in device memory.  Returns n_admissible."""
        if dtype not in (U8, U16):
            raise TypeError("mask must be uint8 or uint16")
        args, n_sets = _draw_args(values, per_value, size, seed, stream, first_draw, n_draws, dtype)
        return Context._draw(self, "ife_sample_positions", mask_ptr, dtype, shape_zyx, out_ptr, MEM_DEVICE, args, n_sets)

    def random_rois_device(self, mask_ptr, dtype, shape_zyx, out_ptr, n_draws, size=(1, 1, 1), values=(),
                           per_value=False, seed=0, stream=0, first_draw=0):
        """sample_positions_device with boxes: out_ptr holds sets * n_draws * 6 int64."""
        if dtype not in (U8, U16):
            raise TypeError("mask must be uint8 or uint16")
        args, n_sets = _draw_args(values, per_value, size, seed, stream, first_draw, n_draws, dtype)
        return Context._draw(self, "ife_random_rois", mask_ptr, dtype, shape_zyx, out_ptr, MEM_DEVICE, args, n_sets)

    def sample_positions(self, mask, n_draws, size=(1, 1, 1), values=(), per_value=False, seed=0, stream=0,
                         first_draw=0):
        """Seeded draws, with replacement, of voxels of a uint8 or uint16 (z, y, x) mask around
        which a box of `size` (x, y, z) fits the volume: (positions (sets, n_draws) int64 linear
        indices, n_admissible (sets,)).  values empty: one set, mask != 0; per_value False: one
        set, mask in values; per_value True: one set per value, drawn from stream + its place.
        Draw first_draw + i depends on (seed, stream, its number) and the mask alone
        (include/ife_hip.h has the definition).  n_draws == 0 gives the counts alone."""
        return _draw_host(self, "ife_sample_positions", (), mask, n_draws, size, values, per_value, seed, stream,
                          first_draw)

    def random_rois(self, mask, n_draws, size, values=(), per_value=False, seed=0, stream=0, first_draw=0):
        """sample_positions as boxes: (rois (sets, n_draws, 6) int64 {x - sx // 2, y - sy // 2,
        z - sz // 2, sx, sy, sz}, n_admissible (sets,))."""
        return _draw_host(self, "ife_random_rois", (6,), mask, n_draws, size, values, per_value, seed, stream,
                          first_draw)

    def extract_rois_device(self, src_ptr, elem_bytes, src_shape_zyx, rois_ptr, n_rois, dst_ptr):
        """Enqueues on the context's stream and waits; src_ptr: the volume, rois_ptr: n_rois * 6
        int64, dst_ptr: n_rois boxes of elem_bytes bytes per element, all in device memory."""
        if int(elem_bytes) not in (1, 2, 4, 8):
            raise TypeError("elements of 1, 2, 4 or 8 bytes are copied (got %d)" % elem_bytes)
        if int(n_rois) < 0:
            raise ValueError("negative count")
        d = _desc(src_shape_zyx, (1.0, 1.0, 1.0))
        self._chk(self._lib.ife_extract_rois(self._h, C.c_void_p(src_ptr or 0), int(elem_bytes), C.byref(d),
                                             C.c_void_p(rois_ptr or 0), int(n_rois), C.c_void_p(dst_ptr or 0),
                                             MEM_DEVICE))

    def extract_rois(self, src, rois):
        """The boxes rois (n, 6) {x, y, z, sx, sy, sz}, all of one size and inside the (z, y, x)
        volume src of any dtype of 1, 2, 4 or 8 bytes, as a new (n, sz, sy, sx) array of that
        dtype.  Bits are copied, nothing is converted."""
        src = np.ascontiguousarray(src)
        if src.ndim != 3:
            raise ValueError("src must be a (z, y, x) volume")
        if src.dtype.itemsize not in (1, 2, 4, 8):
            raise TypeError("elements of 1, 2, 4 or 8 bytes are copied (got %d)" % src.dtype.itemsize)
        rois = np.ascontiguousarray(rois, np.int64).reshape(-1, 6)
        if rois.shape[0] == 0:
            return np.empty((0, 0, 0, 0), src.dtype)
        sx, sy, sz = (int(v) for v in rois[0, 3:])
        if min(sx, sy, sz) < 1:
            raise ValueError("the region's size must be at least 1 on every axis")
        out = np.empty((rois.shape[0], sz, sy, sx), src.dtype)
        d = _desc(src.shape, (1.0, 1.0, 1.0))
        self._chk(self._lib.ife_extract_rois(self._h, src.ctypes.data, src.dtype.itemsize, C.byref(d), rois.ctypes.data,
                                             rois.shape[0], out.ctypes.data, MEM_HOST))
        return out

    # ---- census and coverage: the two questions of ImageBrowser ------------------------------
    def _census(self, values_ptr, n, uniq_ptr, counts_ptr, capacity, mem):
        """One ife_value_census_f32 call; returns (n_unique, n_nan).  Where the outputs are too
        small the IfeError carries the two counts as .n_unique and .n_nan."""
        nu, nn = C.c_int64(-1), C.c_int64(-1)
        try:
            self._chk(self._lib.ife_value_census_f32(self._h, C.c_void_p(values_ptr or 0), int(n),
                                                     C.c_void_p(uniq_ptr or 0), C.c_void_p(counts_ptr or 0),
                                                     int(capacity), C.byref(nu), C.byref(nn), mem))
        except IfeError as e:
            e.n_unique, e.n_nan = nu.value, nn.value
            raise
        return nu.value, nn.value

    def value_census_device(self, values_ptr, n, uniq_ptr=None, counts_ptr=None, capacity=0):
        """Enqueues on the context's stream and waits; values_ptr: n float32, uniq_ptr: capacity
        float32, counts_ptr: capacity uint32, all in device memory.  Returns (n_unique, n_nan);
        capacity 0 without outputs gives the two counts alone."""
        if int(n) <= 0:
            raise ValueError("the element count must be positive")
        if int(capacity) < 0:
            raise ValueError("negative capacity")
        return Context._census(self, values_ptr, n, uniq_ptr, counts_ptr, capacity, MEM_DEVICE)

    def value_census(self, values):
        """The distinct values of a float32 array in ascending order and how often each occurs:
        (uniq float32, counts uint32, n_nan).  NaNs are left out and counted; -0 and +0 are one
        value, reported as +0; any other two elements are one value iff their bits are equal.
        Two library calls, the first for the sizes of the outputs: the array is uploaded and
        sorted twice (value_census_device on a resident array saves the uploads, not the sorts)."""
        values = np.ascontiguousarray(values)
        if values.dtype != np.float32:
            raise TypeError("values must be float32")
        if values.size == 0:
            raise ValueError("the element count must be positive")
        n_unique, n_nan = Context._census(self, values.ctypes.data, values.size, None, None, 0, MEM_HOST)
        uniq, counts = np.empty(n_unique, np.float32), np.empty(n_unique, np.uint32)
        if n_unique:
            Context._census(self, values.ctypes.data, values.size, uniq.ctypes.data, counts.ctypes.data, n_unique,
                            MEM_HOST)
        return uniq, counts, n_nan

    def threshold_mask_device(self, image_ptr, n, low, high, mask_ptr):
        """Enqueues on the context's stream and waits; image_ptr: n float32, mask_ptr: n bytes,
        both in device memory.  Returns the number of ones."""
        low, high = _threshold_args(low, high)
        if int(n) <= 0:
            raise ValueError("the element count must be positive")
        count = C.c_int64()
        self._chk(self._lib.ife_threshold_mask(self._h, C.c_void_p(image_ptr or 0), int(n), low, high,
                                               C.c_void_p(mask_ptr or 0), C.byref(count), MEM_DEVICE))
        return count.value

    def threshold_mask(self, image, low, high):
        """(mask uint8 of the image's shape, count): 1 where low <= image <= high, both ends
        inclusive (itk::BinaryThresholdImageFilter), 0 elsewhere and at NaNs; -0 equals +0."""
        image = np.ascontiguousarray(image)
        if image.dtype != np.float32:
            raise TypeError("image must be float32")
        low, high = _threshold_args(low, high)
        if image.size == 0:
            raise ValueError("the element count must be positive")
        mask = np.empty(image.shape, np.uint8)
        count = C.c_int64()
        self._chk(self._lib.ife_threshold_mask(self._h, image.ctypes.data, image.size, low, high, mask.ctypes.data,
                                               C.byref(count), MEM_HOST))
        return mask, count.value

    def _coverage(self, mask_ptr, dtype, shape_zyx, rois_ptr, n_rois, round_ends, mem):
        ends, n_rounds = _round_ends_arg(round_ends, n_rois)
        d = _desc(shape_zyx, (1.0, 1.0, 1.0))
        visited, hits = np.zeros(n_rounds, np.int64), np.zeros(n_rounds, np.int64)
        region = C.c_int64()
        p64 = C.POINTER(C.c_int64)
        self._chk(self._lib.ife_roi_coverage(self._h, C.c_void_p(mask_ptr or 0), int(dtype), C.byref(d),
                                             C.c_void_p(rois_ptr or 0), int(n_rois), ends, n_rounds,
                                             visited.ctypes.data_as(p64), hits.ctypes.data_as(p64), C.byref(region),
                                             mem))
        return visited, hits, region.value

    def roi_coverage_device(self, mask_ptr, dtype, shape_zyx, rois_ptr, n_rois, round_ends):
        """Enqueues on the context's stream and waits; mask_ptr: the mask of dtype code U8 or U16,
        rois_ptr: n_rois * 6 int64, both in device memory.  Returns (visited, hits, region_size)."""
        if dtype not in (U8, U16):
            raise TypeError("mask must be uint8 or uint16")
        if int(n_rois) < 0:
            raise ValueError("negative count")
        return Context._coverage(self, mask_ptr, dtype, shape_zyx, rois_ptr, n_rois, round_ends, MEM_DEVICE)

    def roi_coverage(self, mask, rois, round_ends):
        """How much of a uint8 or uint16 (z, y, x) mask a growing list of boxes covers.  rois (n, 6)
        {x, y, z, sx, sy, sz}, of any sizes; round r is the union of the boxes before
        round_ends[r] (non-decreasing, at most n, at most 64 rounds).  Returns (visited (rounds,)
        int64 voxels of the union, hits (rounds,) of them with mask != 0, region_size the number
        of voxels with mask != 0)."""
        mask, mdt, mptr = _mask_arg(mask)
        if mask is None or mask.ndim != 3:
            raise ValueError("mask must be a (z, y, x) volume")
        rois = np.ascontiguousarray(rois, np.int64)
        if rois.ndim != 2 or rois.shape[1] != 6:
            raise ValueError("rois must be an (n, 6) array")
        return Context._coverage(self, mptr, mdt, mask.shape, rois.ctypes.data if rois.size else None, rois.shape[0],
                                 round_ends, MEM_HOST)

    def scale_select_device(self, image_ptr, image_dtype, mask_ptr, mask_dtype, shape_zyx, spacing, sigmas,
                            measures, response_ptr, index_ptr=None):
        """Enqueues on the context's stream and waits; response_ptr: [n_measures][nvox] float32,
        index_ptr: the same in uint8 or None, both in device memory (ife_scale_select)."""
        d = _desc(shape_zyx, spacing)
        sig = _sigma_arg(sigmas)
        ms = _scale_measures_arg(measures, len(sigmas))
        self._chk(self._lib.ife_scale_select(
            self._h, C.c_void_p(image_ptr or 0), image_dtype, C.c_void_p(mask_ptr or 0), mask_dtype, C.byref(d), sig,
            len(sigmas), ms, len(ms), C.c_void_p(response_ptr or 0), C.c_void_p(index_ptr or 0), MEM_DEVICE))

    def scale_select(self, image, mask, sigmas, measures, spacing=(1.0, 1.0, 1.0), want_index=True):
        """The maximum over the scales of every measure (ScaleMeasure) and the index of the scale
        that reached it: (response (M, nz, ny, nx) float32, index (M, nz, ny, nx) uint8 or None).
        Index 255 with response 0: no scale had a positive response.  The features are those of
        emphysema_features, with OPT_DIFFERENTIAL at 1 those of differential_features."""
        image, idt = _image_arg(image)
        if image.ndim != 3:
            raise ValueError("image must be a (z, y, x) volume")
        mask, mdt, mptr = _mask_arg(mask)
        ms = _scale_measures_arg(measures, len(sigmas))
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        response = np.empty((len(ms),) + image.shape, np.float32)
        index = np.empty((len(ms),) + image.shape, np.uint8) if want_index else None
        self._chk(self._lib.ife_scale_select(
            self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig, len(sigmas), ms, len(ms),
            response.ctypes.data, index.ctypes.data if want_index else None, MEM_HOST))
        return response, index

    def bag_image_dense_stream(self, image, mask, sigmas, size, edges, gen_mask=None,
                               spacing=(1.0, 1.0, 1.0), values="frequencies", block_mb=0):
        """The bag of bag_image_dense as a stream of row blocks: a generator of
        (row0, ndarray[n_rows, n_sigmas*8, n_edges+1]), float32 frequencies (an empty histogram is
        NaN) or uint32 counts (values="counts").  A block is a run of whole centre planes of at
        most block_mb MiB (0: from the scratch budget); while one is copied the next is counted."""
        if mask is None:
            raise TypeError("a mask is required")
        if values not in ("counts", "frequencies", BAG_COUNTS, BAG_FREQUENCIES):
            raise ValueError("values must be 'counts' or 'frequencies'")
        freq = values in ("frequencies", BAG_FREQUENCIES)
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        gen_mask, gdt, gptr = _mask_arg(gen_mask)
        edges = np.ascontiguousarray(edges, np.float32)
        ne = edges.shape[1]
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        n, cap = C.c_int64(), C.c_int64()
        self._chk(self._lib.ife_bag_dense_stream_begin(
            self._h, image.ctypes.data, idt, mptr, mdt, gptr, gdt, C.byref(d), sig, len(sigmas),
            _size_arg(size), edges.ctypes.data, ne, BAG_FREQUENCIES if freq else BAG_COUNTS,
            int(block_mb), C.byref(n), C.byref(cap), MEM_HOST))
        try:
            while True:
                rows = np.empty((max(cap.value, 1), 8 * len(sigmas), ne + 1), np.float32 if freq else np.uint32)
                row0, got = C.c_int64(), C.c_int64()
                self._chk(self._lib.ife_bag_dense_stream_next(self._h, rows.ctypes.data, rows.shape[0],
                                                              C.byref(row0), C.byref(got)))
                if got.value == 0:
                    break
                yield row0.value, rows[:got.value]
        finally:
            self._chk(self._lib.ife_bag_dense_stream_end(self._h))

    def samples(self, n_columns):
        return Samples(self, n_columns)


class Multi:
    """``ife_multi``: the Z-slab engine over several devices of one process (peer copies)."""

    def __init__(self, devices):
        self._lib = load_library()
        devs = (C.c_int * len(devices))(*[int(d) for d in devices])
        h = C.c_void_p()
        rc = self._lib.ife_multi_create(devs, len(devices), C.byref(h))
        if rc != OK:
            raise IfeError(rc, self._lib.ife_multi_last_error(None).decode())
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.ife_multi_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _chk(self, rc):
        if rc < 0:
            raise IfeError(rc, self._lib.ife_multi_last_error(self._h).decode())

    def set_option(self, option, value):
        self._chk(self._lib.ife_multi_set_option(self._h, int(option), int(value)))

    def _features(self, call, image, mask, sigmas, spacing, layout):
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        shp = image.shape + (8,) if layout == INTERLEAVED else (8,) + image.shape
        out = np.empty((len(sigmas),) + shp, np.float32)
        self._chk(call(self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig,
                       len(sigmas), out.ctypes.data, layout))
        return out

    def _features_stream(self, begin, image, mask, sigmas, spacing, layout):
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        shp = image.shape + (8,) if layout == INTERLEAVED else (8,) + image.shape
        self._chk(begin(self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig, len(sigmas), layout))
        try:
            for k in range(len(sigmas)):
                out = np.empty(shp, np.float32)
                self._chk(self._lib.ife_multi_emphysema_features_fetch(self._h, k, out.ctypes.data))
                yield out
        finally:
            self._chk(self._lib.ife_multi_emphysema_features_end(self._h))

    def emphysema_features(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        return self._features(self._lib.ife_multi_emphysema_features, image, mask, sigmas, spacing, layout)

    def emphysema_features_stream(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        """Generator over the scales: one upload and prepass, every scale enqueued on every
        device, then one blocking fetch per scale (ife_multi_emphysema_features_begin / _fetch /
        _end) -- the scale loop of tools/ExtractFeatures.cxx:132-154 over several devices."""
        return self._features_stream(self._lib.ife_multi_emphysema_features_begin, image, mask, sigmas, spacing,
                                     layout)

    def differential_features(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        """Context.differential_features over the devices of the engine (bit for bit)."""
        return self._features(self._lib.ife_multi_differential_features, image, mask, sigmas, spacing, layout)

    def differential_features_stream(self, image, mask, sigmas, spacing=(1.0, 1.0, 1.0), layout=INTERLEAVED):
        """emphysema_features_stream with every scale that of differential_features."""
        return self._features_stream(self._lib.ife_multi_differential_features_begin, image, mask, sigmas,
                                     spacing, layout)


class Samples:
    """``ife_samples``: one growing device-resident column per (scale, feature), the
    `samples` vector of tools/DetermineHistogramBinEdges_MultiScaleEigenvalueFeatures.cxx."""

    def __init__(self, ctx, n_columns):
        self._ctx, self._lib = ctx, ctx._lib
        self.n_columns = int(n_columns)
        h = C.c_void_p()
        ctx._chk(self._lib.ife_samples_create(ctx._h, self.n_columns, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None) and getattr(self._ctx, "_h", None):
            self._lib.ife_samples_destroy(self._h)
        self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def count(self, column=0):
        n = C.c_int64()
        self._ctx._chk(self._lib.ife_samples_count(self._h, int(column), C.byref(n)))
        return n.value

    def clear(self):
        self._ctx._chk(self._lib.ife_samples_clear(self._h))

    @staticmethod
    def _fg(foreground):
        fg = np.ascontiguousarray(foreground, np.uint32).ravel()
        return fg, (fg.ctypes.data if fg.size else None)

    def add_features(self, first_column, features, mask=None, foreground=(1,), indices=None,
                     layout=INTERLEAVED):
        """features: (nz, ny, nx, ncomp) interleaved or (ncomp, nz, ny, nx) planar, host."""
        f = np.ascontiguousarray(features, np.float32)
        ncomp = f.shape[-1] if layout == INTERLEAVED else f.shape[0]
        nvox = f.size // ncomp
        fg, fgp = self._fg(foreground)
        mptr, mdt, iptr, ni = None, U8, None, 0
        if indices is not None:
            indices = np.ascontiguousarray(indices, np.int64).ravel()
            iptr, ni = indices.ctypes.data, indices.size
        else:
            mask, mdt, mptr = _mask_arg(mask)
        self._ctx._chk(self._lib.ife_samples_add_features(
            self._ctx._h, self._h, int(first_column), f.ctypes.data, layout, ncomp, mptr, mdt, nvox,
            fgp, fg.size, iptr, ni, MEM_HOST))

    def add_image(self, image, mask, sigmas, foreground=(1,), indices=None,
                  spacing=(1.0, 1.0, 1.0)):
        """One image of the tool's loop: features at every scale stay on the device."""
        image, idt = _image_arg(image)
        mask, mdt, mptr = _mask_arg(mask)
        d = _desc(image.shape, spacing)
        sig = _sigma_arg(sigmas)
        fg, fgp = self._fg(foreground)
        iptr, ni = None, 0
        if indices is not None:
            indices = np.ascontiguousarray(indices, np.int64).reshape(len(sigmas), -1)
            iptr, ni = indices.ctypes.data, indices.shape[1]
        self._ctx._chk(self._lib.ife_samples_add_image(
            self._ctx._h, self._h, image.ctypes.data, idt, mptr, mdt, C.byref(d), sig, len(sigmas),
            fgp, fg.size, iptr, ni, MEM_HOST))

    def add_image_device(self, image_ptr, image_dtype, mask_ptr, mask_dtype, shape_zyx, sigmas,
                         foreground=(1,), spacing=(1.0, 1.0, 1.0)):
        d = _desc(shape_zyx, spacing)
        sig = _sigma_arg(sigmas)
        fg, fgp = self._fg(foreground)
        self._ctx._chk(self._lib.ife_samples_add_image(
            self._ctx._h, self._h, C.c_void_p(image_ptr), image_dtype, C.c_void_p(mask_ptr),
            mask_dtype, C.byref(d), sig, len(sigmas), fgp, fg.size, None, 0, MEM_DEVICE))

    def sort(self):
        self._ctx._chk(self._lib.ife_samples_sort(self._ctx._h, self._h))

    def equalized_edges(self, nbins):
        """(n_columns, nbins-1) float32: one row per (scale, feature) as the tool writes them."""
        out = np.empty((self.n_columns, max(int(nbins) - 1, 0)), np.float32)
        self._ctx._chk(self._lib.ife_samples_equalized_edges(self._ctx._h, self._h, int(nbins),
                                                             out.ctypes.data))
        return out

    def column(self, column):
        out = np.empty(self.count(column), np.float32)
        self._ctx._chk(self._lib.ife_samples_read_column(self._ctx._h, self._h, int(column),
                                                         out.ctypes.data, out.size))
        return out
