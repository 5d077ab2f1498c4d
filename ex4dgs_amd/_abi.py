"""The one Python mirror of include/*.h: every structure, every prototype, the loader of libex4d_hip.so and the three helpers the
binding modules share.  tests/test_cpu_abi.py reads the structures and the table below against the headers -- names, return types,
every parameter in order, every field -- so a header change that is not repeated here fails on the CPU instead of mis-calling.

A new entry point is a line in PROTOTYPES (and its structure here); nothing else sets a prototype.
"""
import contextlib
import ctypes as C
import os

import torch

_CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
# EX4D_HIP_LIB: developer override (a variant build of the same sources, e.g. tools/dev/spill_probe.py); the product loads the in-tree library
_LIB_PATH = os.environ.get("EX4D_HIP_LIB") or os.path.join(_CSRC, "libex4d_hip.so")
_lib = None

RADAM_MAX_WINDOWS = 8        # EX4D_RADAM_MAX_WINDOWS
TRAINER_PARAMS = 15          # EX4D_TRAINER_PARAMS


def _all(ctype, *names):
    return [(n, ctype) for n in names]


i32, i64, f32, f64, vp, cint, size, text = C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_void_p, C.c_int, C.c_size_t, C.c_char_p
P = C.POINTER


# ---- ex4d_rasterizer.h
class Ex4dParams(C.Structure):
    _fields_ = [*_all(i32, "P", "D", "M", "W", "H"),
                *_all(f32, "tanfovx", "tanfovy", "kernel_size", "scale_modifier", "min_depth", "max_depth"),
                *_all(i32, "prefiltered", "debug", "prepare_backward", "instance_capacity", "assume_no_flow", "reserved")]


ALLOC_FN = C.CFUNCTYPE(vp, vp, size)                     # ex4d_alloc_fn


class Ex4dSplitSH(C.Structure):
    _fields_ = [("dc", vp * 2), ("rest", vp * 2), ("n_static", i32)]


Ex4dSplitSHGrad = Ex4dSplitSH                            # the same layout without the const


class Ex4dGeomLayout(C.Structure):
    _fields_ = _all(size, "records", "cov3D", "clamped", "tiles_touched", "depth_order", "sorted_offsets", "rects", "total")


class Ex4dBinningLayout(C.Structure):
    _fields_ = _all(size, "point_list", "tile_ids", "qlist", "qcount", "total")


class Ex4dImgLayout(C.Structure):
    _fields_ = _all(size, "final_T", "n_contrib", "ranges", "total")


GeomLayout, BinningLayout, ImgLayout = Ex4dGeomLayout, Ex4dBinningLayout, Ex4dImgLayout


# ---- ex4d_attributes.h
class Ex4dAttrParams(C.Structure):
    _fields_ = [*_all(i32, "Ns", "Nd", "K", "k"), *_all(f32, "t", "duration", "delta", "h00", "h10", "h01", "h11", "tau", "var_min")]


# ---- ex4d_optim.h
class Ex4dRadamTensor(C.Structure):
    _fields_ = [*_all(vp, "param", "grad", "exp_avg", "exp_avg_sq"), ("numel", i64), ("lr", f64), ("step", i64),
                ("nan_to_num", i32), ("reserved", i32)]


class Ex4dRadamSlicedTensor(C.Structure):
    _fields_ = [*_all(vp, "param", "exp_avg", "exp_avg_sq"), ("rows", i64), ("K", i32), ("C", i32), ("lr", f64), ("step", i64),
                ("n_windows", i32), ("first", i32 * RADAM_MAX_WINDOWS), ("count", i32 * RADAM_MAX_WINDOWS),
                ("grad", vp * RADAM_MAX_WINDOWS), ("first_dev", vp)]


class Ex4dRadamSlicedRegTensor(C.Structure):
    _fields_ = [("t", Ex4dRadamSlicedTensor), ("reg_kind", i32), ("reserved", i32), ("reg_weight", f64), ("reg_rows", i64)]


# ---- ex4d_densify.h
class Ex4dDensifyPlanGroup(C.Structure):
    _fields_ = [("n", i64), *_all(vp, "stats", "scaling", "opacity", "xyz"), ("xyz_width", i32), ("use_screen", i32),
                *_all(f32, "grad_thr", "dense_scale", "big_scale", "screen_size", "min_opacity", "l1_thres", "max_ssim"),
                ("reserved", i32), *_all(vp, "map", "counts", "scratch")]


class Ex4dDensifyTensor(C.Structure):
    _fields_ = [("src", vp), ("dst", vp), ("rows", i64), ("dst_rows", i64), *_all(i32, "width", "planes", "rule", "group"),
                ("aux0", vp), ("aux1", vp), ("value", f32), ("reserved", i32)]


class Ex4dDensifyApplyGroup(C.Structure):
    _fields_ = [("map", vp), ("child_stride", i64), ("n_split", i64), *_all(vp, "split_z", "split_c1", "split_c0", "clone_c1", "clone_c0"),
                *_all(f32, "min_len", "center_lo", "center_hi", "split_div")]


class Ex4dGrowthClassify(C.Structure):
    _fields_ = [("n", i64), *_all(vp, "score", "result", "disp", "stats"), ("motion_abs", f32), ("min_abs", f32),
                *_all(vp, "map", "counts", "selected", "counts_out", "scratch")]


class Ex4dGrowthTensor(C.Structure):
    _fields_ = [*_all(vp, "old", "dst", "src0", "src1"), ("old_rows", i64), ("width", i32), ("rule", i32)]


class Ex4dGrowthAppend(C.Structure):
    _fields_ = [("selected", vp), ("n_new", i64), ("n_static", i64), ("stats", vp), ("K", i32),
                *_all(f32, "interval", "max_dur", "b_scale", "time_shift", "time_pad", "center_lo", "center_hi")]


# ---- ex4d_trainer.h
class Ex4dTrainerConfig(C.Structure):
    _fields_ = [*_all(i32, "Ns", "Nd", "K", "W", "H", "sh_degree"), *_all(f32, "tanfovx", "tanfovy", "kernel_size", "min_depth", "max_depth"),
                *_all(f64, "duration", "interval", "time_shift", "var_pad"), ("lambda_dssim", f32), ("window", f32 * 11),
                ("lr", f64 * TRAINER_PARAMS), *_all(f64, "beta1", "beta2", "eps"), ("optimizer", i32)]


class Ex4dTrainerStepOptions(C.Structure):
    _fields_ = [*_all(i32, "l1_accum", "skip_optimizer", "stats_flags", "nan_census"), *_all(vp, "stats_s", "stats_d")]


class Ex4dTrainerReport(C.Structure):
    _fields_ = [("loss", f32), *_all(i32, "nan_static", "nan_dynamic", "reserved")]


def _status(name, *argtypes):
    """An entry point whose int return is a status: 0, or an error whose text the header's *_last_error holds (see call)."""
    return name, cint, argtypes, True


def _value(name, restype, *argtypes):
    """An entry point that returns a value (or nothing: None)."""
    return name, restype, argtypes, False


_fwd_tail = (ALLOC_FN, vp) * 3 + (vp,) * 6 + (vp, P(i32))      # three allocation callbacks, six outputs, stream, num_rendered
# header -> (its *_last_error, its prototypes in header order); a pointer to data is c_void_p, to a structure POINTER(its mirror)
PROTOTYPES = {
    "ex4d_rasterizer.h": ("ex4d_last_error", (
        _value("ex4d_last_error", text),
        _value("ex4d_abi_version", cint),
        _value("ex4d_target_arch", text),
        _status("ex4d_forward", P(Ex4dParams), *[vp] * 13, *_fwd_tail),
        _status("ex4d_backward", P(Ex4dParams), i32, *[vp] * 32),
        _value("ex4d_backward_scratch_bytes", size, i32),
        _status("ex4d_forward_split_sh", P(Ex4dParams), *[vp] * 3, P(Ex4dSplitSH), *[vp] * 8, *_fwd_tail),
        _status("ex4d_backward_split_sh", P(Ex4dParams), i32, *[vp] * 3, P(Ex4dSplitSH), *[vp] * 21, P(Ex4dSplitSHGrad), *[vp] * 5),
        _status("ex4d_mark_visible", i32, vp, vp, vp, f32, f32, vp, vp),
        _value("ex4d_geom_bytes", size, i32),
        _value("ex4d_binning_bytes", size, i32, i32, i32),
        _value("ex4d_img_bytes", size, i32, i32),
        _value("ex4d_geom_layout", None, i32, P(Ex4dGeomLayout)),
        _value("ex4d_binning_layout", None, i32, i32, i32, P(Ex4dBinningLayout)),
        _value("ex4d_img_layout", None, i32, i32, P(Ex4dImgLayout)),
        _status("ex4d_set_option", text, cint),
        _value("ex4d_get_option", cint, text),
        _status("ex4d_debug_bwd_stats", P(C.c_ulonglong), cint),
        _status("ex4d_debug_bwd_stats16", P(C.c_ulonglong), cint),
        _status("ex4d_debug_rows_prof", P(C.c_ulonglong), cint),
        _status("ex4d_debug_sample_sort", P(C.c_ulonglong), cint),
        _value("ex4d_profile_enable", None, cint),
        _value("ex4d_profile_read", cint, cint, P(f32), P(text), cint))),
    "ex4d_attributes.h": ("ex4d_attributes_last_error", (
        _value("ex4d_attributes_last_error", text),
        _status("ex4d_attributes_forward", P(Ex4dAttrParams), *[vp] * 21),
        _status("ex4d_attributes_backward", P(Ex4dAttrParams), *[vp] * 28),
        _status("ex4d_attributes_backward_sliced", P(Ex4dAttrParams), *[vp] * 27, P(i32), vp),
        _status("ex4d_attr_time_scalars", i32, f64, f64, f64, f64, i32, i32, i32, f64, P(Ex4dAttrParams)),
        _status("ex4d_attributes_forward_ex", P(Ex4dAttrParams), i32, *[vp] * 21),
        _status("ex4d_attributes_backward_ex", P(Ex4dAttrParams), i32, *[vp] * 29),
        _status("ex4d_attributes_backward_sliced_ex", P(Ex4dAttrParams), i32, *[vp] * 28, P(i32), vp),
        _value("ex4d_motion_last_error", text),
        _status("ex4d_motion_forward", P(Ex4dAttrParams), P(Ex4dAttrParams), i32, i32, *[vp] * 5, i32, i32, f32, vp, vp),
        _status("ex4d_motion_backward", P(Ex4dAttrParams), P(Ex4dAttrParams), i32, i32, *[vp] * 5, i32, i32, f32, *[vp] * 5, P(i32), vp))),
    "ex4d_loss.h": ("ex4d_loss_last_error", (
        _value("ex4d_loss_last_error", text),
        _value("ex4d_l1_ssim_scratch_floats", size, i32, i32),
        _status("ex4d_l1_ssim_forward", i32, i32, i32, vp, vp, f32, *[vp] * 7),
        _status("ex4d_l1_ssim_backward", i32, i32, i32, vp, vp, f32, *[vp] * 5),
        _status("ex4d_l1_ssim_forward_u8", i32, i32, vp, vp, i32, vp, f32, *[vp] * 7),
        _status("ex4d_l1_ssim_backward_u8", i32, i32, vp, vp, i32, vp, f32, *[vp] * 5),
        _value("ex4d_frame_metrics_scratch_floats", size, i32, i32),
        _status("ex4d_frame_metrics", i32, i32, vp, vp, vp, i32, *[vp] * 4),
        _status("ex4d_frame_metrics_u8", i32, i32, vp, vp, i32, vp, vp, i32, *[vp] * 4),
        _value("ex4d_resize_u8_table_words", size, i32, i32, i32),
        _status("ex4d_resize_u8_table", i32, i32, i32, vp),
        _value("ex4d_resize_u8_scratch_bytes", size, i32, i32, i32, i32),
        _status("ex4d_resize_u8", i32, i32, i32, i32, i32, *[vp] * 6),
        _value("ex4d_flow_loss_scratch_floats", size, i32, i32),
        _status("ex4d_flow_loss_forward", i32, i32, vp, vp, i32, f32, vp, i32, f32, *[vp] * 4),
        _status("ex4d_flow_loss_backward", i32, i32, vp, vp, i32, f32, vp, i32, f32, *[vp] * 4),
        _value("ex4d_depth_loss_scratch_bytes", size, i32, i32),
        _status("ex4d_depth_loss_forward", i32, i32, vp, vp, i32, f32, vp, i32, f32, f32, i32, f32, *[vp] * 4),
        _status("ex4d_depth_loss_backward", i32, i32, vp, vp, i32, f32, vp, i32, i32, f32, *[vp] * 4),
        _value("ex4d_frame_skssim_scratch_floats", size, i32, i32),
        _status("ex4d_frame_skssim", i32, i32, vp, vp, i32, *[vp] * 3),
        _status("ex4d_frame_skssim_u8", i32, i32, vp, vp, i32, vp, i32, *[vp] * 3))),
    "ex4d_optim.h": ("ex4d_optim_last_error", (
        _value("ex4d_optim_last_error", text),
        _status("ex4d_radam_step", P(Ex4dRadamTensor), i32, f64, f64, f64, vp),
        _status("ex4d_radam_step_sliced", P(Ex4dRadamSlicedTensor), i32, f64, f64, f64, vp),
        _status("ex4d_radam_step_sliced_reg", P(Ex4dRadamSlicedRegTensor), i32, f64, f64, f64, vp),
        _value("ex4d_radam_sliced_reg_rows", i32, i32, i32))),
    "ex4d_knn.h": ("ex4d_knn_last_error", (
        _value("ex4d_knn_last_error", text),
        _value("ex4d_dist2_scratch_bytes", size, i32),
        _status("ex4d_dist2", i32, vp, vp, vp, vp))),
    "ex4d_densify.h": ("ex4d_densify_last_error", (
        _status("ex4d_densify_stats", vp, i64, vp, i64, vp, vp, vp, f32, i32, vp),
        _status("ex4d_densify_stats_merge", vp, vp, i32, i64, vp, vp),
        _status("ex4d_nan_any", vp, i64, vp, i64, vp, vp),
        _value("ex4d_densify_scratch_bytes", size, i64),
        _status("ex4d_densify_plan", i32, P(Ex4dDensifyPlanGroup), vp),
        _status("ex4d_densify_apply", P(Ex4dDensifyTensor), i32, P(Ex4dDensifyApplyGroup), vp),
        _value("ex4d_densify_last_error", text),
        _status("ex4d_growth_scores", vp, vp, vp, vp, i64, vp, vp),
        _value("ex4d_growth_select_scratch_bytes", size),
        _status("ex4d_growth_select", vp, i64, f32, vp, vp, vp),
        _status("ex4d_growth_classify", P(Ex4dGrowthClassify), vp),
        _status("ex4d_growth_append", P(Ex4dGrowthTensor), i32, P(Ex4dGrowthAppend), vp),
        _status("ex4d_growth_extrapolate", vp, vp, i64, i32, i32, i32, i32, vp),
        _status("ex4d_growth_expand_opacity", vp, vp, vp, vp, i64, f32, f32, f32, vp),
        _status("ex4d_growth_adjust_opacity", vp, vp, vp, vp, i64, f32, f32, vp))),
    "ex4d_regularizers.h": ("ex4d_reg_last_error", (
        _value("ex4d_reg_last_error", text),
        _value("ex4d_reg_scratch_bytes", size),
        _status("ex4d_reg_forward", vp, i64, vp, vp, i64, i32, f64, f64, f64, vp, vp, vp),
        _status("ex4d_reg_backward", vp, vp, i64, vp, vp, vp, vp, i64, i32, f64, f64, f64, vp, i32, vp),
        _status("ex4d_reg_backward_range", i32, vp, i64, i32, i64, i64, vp, f64, i32, vp))),
    "ex4d_trainer.h": ("ex4d_trainer_last_error", (                  # Ex4dTrainer * is opaque: c_void_p
        _value("ex4d_trainer_last_error", text),
        _value("ex4d_trainer_create", vp, P(Ex4dTrainerConfig), P(vp)),
        _value("ex4d_trainer_destroy", None, vp),
        _value("ex4d_trainer_time_scalars", None, P(Ex4dTrainerConfig), f64, P(Ex4dAttrParams)),
        _status("ex4d_trainer_step", vp, f64, *[vp] * 6, P(i32)),
        _status("ex4d_trainer_step_ex", vp, f64, *[vp] * 6, P(i32), P(Ex4dTrainerStepOptions)),
        _status("ex4d_trainer_step_u8", vp, f64, *[vp] * 5, i32, vp, vp, P(i32), P(Ex4dTrainerStepOptions)),
        _status("ex4d_trainer_report", vp, P(Ex4dTrainerReport)),
        _status("ex4d_trainer_set_lr", vp, P(f64)),
        _status("ex4d_trainer_set_sh_degree", vp, i32),
        _status("ex4d_trainer_set_async", vp, i32),
        _value("ex4d_trainer_replays", i64, vp),
        _status("ex4d_trainer_set_interp", vp, i32),
        _status("ex4d_trainer_set_regularizers", vp, f64, f64, f64),
        _value("ex4d_trainer_output", vp, vp, i32),
        _value("ex4d_trainer_grad", vp, vp, i32, P(i32)),
        _status("ex4d_trainer_read", vp, i32, vp, size, vp),
        _status("ex4d_trainer_write", vp, i32, vp, size, vp),
        _status("ex4d_trainer_get_step", vp, P(i64)),
        _status("ex4d_trainer_set_step", vp, i64),
        _value("ex4d_trainer_bytes", size, vp))),
}
# status function -> the *_last_error of its header
_LAST_ERROR = {name: err for err, protos in PROTOTYPES.values() for name, _, _, is_status in protos if is_status}
# the motion entry points are declared in ex4d_attributes.h and keep an error text of their own
_LAST_ERROR.update({name: "ex4d_motion_last_error" for name in _LAST_ERROR if name.startswith("ex4d_motion_")})


def exports(header):
    """The names `header` declares, in its order (the EXPORTS of the module that binds it)."""
    return tuple(name for name, _, _, _ in PROTOTYPES[header][1])


def library_path():
    return _LIB_PATH


def load():
    """dlopen libex4d_hip.so (built in-tree by ex4dgs_amd.build) and bind every prototype of the table; raises if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(f"{_LIB_PATH} not found: build it with `python -m ex4dgs_amd.build` "
                           "(there is no CPU / PyTorch fallback for the rasterizer)")
    lib = C.CDLL(_LIB_PATH)
    for _, protos in PROTOTYPES.values():
        for name, restype, argtypes, _ in protos:
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, list(argtypes)
    _lib = lib
    return lib


def call(name, *args):
    """Call a status function; a refused call raises the text its header's *_last_error holds for it."""
    err = _LAST_ERROR[name]                    # KeyError: not a status function -- call it on load() and read its value
    lib = load()
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise RuntimeError(getattr(lib, err)().decode() or f"{name} failed with status {rc}")


def ptr(t):
    """The data pointer of a tensor; None (NULL) for an absent or empty one."""
    return None if t is None or t.numel() == 0 else t.data_ptr()


@contextlib.contextmanager
def stream(device):
    """Makes `device` current (the library works on the current HIP device) and yields its current stream as the void * the ABI takes."""
    with torch.cuda.device(device):
        yield C.c_void_p(torch.cuda.current_stream().cuda_stream)
