"""The differential path over several devices, across the layers that need no device: the C
header declares the stage calls with an order per job, the jet stage and the two engine calls, the
library exports them, and the Python binding carries them beside everything it carried before."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FUNCTIONS = ["ife_stage_z_sweep_order", "ife_stage_z_combine_order", "ife_stage_z_fused_order",
                 "ife_stage_jet_features", "ife_multi_differential_features",
                 "ife_multi_differential_features_begin"]
NEW_CONTEXT_METHODS = ["stage_z_sweep_order", "stage_z_combine_order", "stage_z_fused_order", "stage_jet_features"]
NEW_MULTI_METHODS = ["differential_features", "differential_features_stream"]
OLD_CONTEXT_METHODS = [
    "set_stream", "set_option", "reserve", "synchronize", "kernel_times", "measure_stream", "reset_kernel_times",
    "eigenvalues", "eigenvalue_features", "hessian3d", "gradient_magnitude", "normalized_gaussian_convolution",
    "differential_normalized_convolution", "emphysema_features", "normalized_convolution_jet",
    "differential_features", "emphysema_features_stream", "scale_stream", "deflate_bound", "deflate",
    "deflate_device", "fd_hessian_features", "fd_gradient_features", "mask_image_f64", "signed_distance_map",
    "expected_distance", "signed_distance_map_device", "emphysema_features_device",
    "differential_features_device", "normalized_convolution_jet_device", "fd_hessian_features_device",
    "stage_prepare", "stage_recursive_gaussian", "stage_recursive_gaussian_order",
    "stage_recursive_gaussian_batch", "stage_features", "stage_z_ck_bytes", "stage_z_sweep", "stage_z_combine",
    "stage_z_fused", "stage_recursive_gaussian_quotient", "sort_f32", "sort_f32_device", "equalized_edges",
    "dense_histogram", "roi_histograms", "bag_image", "dense_rois", "dense_roi_histograms", "bag_image_dense",
    "bag_image_dense_stream", "samples", "close"]
OLD_MULTI_METHODS = ["close", "set_option", "emphysema_features", "emphysema_features_stream"]


def header_text():
    return open(os.path.join(ROOT, "include", "ife_hip.h")).read()


def test_header_declares_the_new_functions():
    text = header_text()
    for name in NEW_FUNCTIONS:
        assert re.search(r"^int %s\(" % name, text, re.M), name
    # the order goes in behind the sigmas, one per job
    for name in NEW_FUNCTIONS[:3]:
        decl = text[text.index("int %s(" % name):]
        decl = decl[:decl.index(";")]
        assert re.search(r"const double \*sigmas,\s*const int \*orders", decl), name
    # the existing calls keep their signatures
    for name in ("ife_stage_z_sweep", "ife_stage_z_combine", "ife_stage_z_fused"):
        decl = text[text.index("int %s(" % name):]
        assert "orders" not in decl[:decl.index(";")], name


def test_header_keeps_the_options():
    text = header_text()
    body = text[text.index("/* Options for ife_ctx_set_option */"):text.index("} ife_option;")]
    values = sorted(int(v) for v in re.findall(r"\bIFE_OPT_[A-Z_]+ = (\d+)", body))
    assert values == list(range(1, 14)), "no new option"


def test_library_exports_the_new_functions(ife):
    lib = ife.load_library()
    for name in NEW_FUNCTIONS:
        assert name in ife.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.ife_multi_differential_features.argtypes == lib.ife_multi_emphysema_features.argtypes


def test_python_methods(ife):
    for name in NEW_CONTEXT_METHODS + OLD_CONTEXT_METHODS:
        assert callable(getattr(ife.Context, name, None)), "Context.%s" % name
    for name in NEW_MULTI_METHODS + OLD_MULTI_METHODS:
        assert callable(getattr(ife.Multi, name, None)), "Multi.%s" % name
