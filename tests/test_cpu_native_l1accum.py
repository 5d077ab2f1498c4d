"""The compiled trainer's l1_accum / statistics / resizing interface without a GPU: the library exports the new entry points,
ex4dgs_amd/_abi.py mirrors the two new structures in the header's field order, and the calls that cannot be served are refused with
the header's own message before any HIP call is made."""
import ctypes
import inspect
import os
import re

import pytest

from ex4dgs_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_TRAINER = ("ex4d_trainer_step_ex", "ex4d_trainer_report", "ex4d_trainer_write", "ex4d_trainer_get_step", "ex4d_trainer_set_step")


def _struct_fields(header, name):
    """Field names of `typedef struct name { ... } name;` in declaration order (comments stripped)."""
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    body = re.search(rf"typedef struct {name}\s*\{{(.*?)\}}\s*{name}\s*;", text, flags=re.S).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        ctype, names = re.fullmatch(r"(?:const\s+)?(\w+)\s+(.*)", decl, flags=re.S).groups()
        fields += [(n.strip().lstrip("*").strip(), ctype, n.strip().startswith("*")) for n in names.split(",")]
    return fields


def test_the_library_exports_the_new_entry_points():
    from ex4dgs_amd import build, densify, native_trainer
    handle = ctypes.CDLL(build.build())
    for name in NEW_TRAINER + ("ex4d_nan_any",):
        assert hasattr(handle, name), name
    assert set(NEW_TRAINER) <= set(native_trainer.EXPORTS) and "ex4d_nan_any" in densify.EXPORTS
    status = {n for _, protos in _abi.PROTOTYPES.values() for n, _, _, is_status in protos if is_status}
    assert set(NEW_TRAINER) | {"ex4d_nan_any"} <= status, "every new int return is a status: values go through out-pointers"


def test_the_two_new_structures_mirror_the_header():
    opts = _struct_fields("ex4d_trainer.h", "Ex4dTrainerStepOptions")
    assert [f for f, _, _ in opts] == ["l1_accum", "skip_optimizer", "stats_flags", "nan_census", "stats_s", "stats_d"]
    assert [f for f, _ in _abi.Ex4dTrainerStepOptions._fields_] == [f for f, _, _ in opts]
    for (field, got), (_, ctype, pointer) in zip(_abi.Ex4dTrainerStepOptions._fields_, opts):
        assert got is (ctypes.c_void_p if pointer else {"int32_t": ctypes.c_int32}[ctype]), field
    assert ctypes.sizeof(_abi.Ex4dTrainerStepOptions) == 4 * 4 + 2 * ctypes.sizeof(ctypes.c_void_p)
    assert _abi.Ex4dTrainerStepOptions.stats_s.offset == 16
    rep = _struct_fields("ex4d_trainer.h", "Ex4dTrainerReport")
    assert [f for f, _, _ in rep] == ["loss", "nan_static", "nan_dynamic", "reserved"]
    assert [(f, t) for f, t in _abi.Ex4dTrainerReport._fields_] == [("loss", ctypes.c_float), ("nan_static", ctypes.c_int32),
                                                                    ("nan_dynamic", ctypes.c_int32), ("reserved", ctypes.c_int32)]
    assert ctypes.sizeof(_abi.Ex4dTrainerReport) == 16


def test_unservable_calls_are_refused_with_the_headers_message_before_any_hip_call():
    lib = _abi.load()
    opt = _abi.Ex4dTrainerStepOptions()
    with pytest.raises(RuntimeError) as e:
        _abi.call("ex4d_trainer_step_ex", None, 0.0, None, None, None, None, None, None, None, ctypes.byref(opt))
    assert str(e.value) == lib.ex4d_trainer_last_error().decode() != ""
    with pytest.raises(RuntimeError) as e:
        _abi.call("ex4d_trainer_write", None, 200, None, 0, None)
    assert str(e.value) == lib.ex4d_trainer_last_error().decode() != ""
    for name, args in (("ex4d_trainer_report", (None, None)), ("ex4d_trainer_get_step", (None, None)), ("ex4d_trainer_set_step", (None, 0))):
        with pytest.raises(RuntimeError) as e:
            _abi.call(name, *args)
        assert str(e.value) == lib.ex4d_trainer_last_error().decode() != "", name
    host = (ctypes.c_float * 8)()                    # never dereferenced: the flags pointer is looked at first
    with pytest.raises(RuntimeError) as e:
        _abi.call("ex4d_nan_any", ctypes.addressof(host), 8, None, 0, None, None)
    assert str(e.value) == lib.ex4d_densify_last_error().decode() != "" and "nan_any" in str(e.value)
    with pytest.raises(RuntimeError, match="nan_any"):
        _abi.call("ex4d_nan_any", None, 8, None, 0, ctypes.addressof(host), None)      # a non-empty array without a pointer


def test_native_trainer_step_keeps_its_positional_arguments_and_adds_keyword_only_options():
    from ex4dgs_amd import densify, growth
    from ex4dgs_amd.native_trainer import NativeTrainer
    params = inspect.signature(NativeTrainer.step).parameters
    assert list(params)[:5] == ["self", "cam", "bg", "t", "gt_image"]
    defaults = {"l1_accum": False, "stats": None, "densify_stats": True, "prune_stats": True, "apply_optimizer": True, "nan_census": False}
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default, name
    for method in ("report", "begin_density_control", "rebind_parameters"):
        assert callable(getattr(NativeTrainer, method))
    assert "NativeTrainer" in inspect.getsource(densify._opt_state) and "NativeTrainer" in inspect.getsource(densify._rebind)
    assert "NativeTrainer" in inspect.getsource(densify._prepare) and "NativeTrainer" in growth.__doc__
