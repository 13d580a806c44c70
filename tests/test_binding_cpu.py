"""The ctypes structures and constants _lib.py generates from include/espnet_amd.h against the
host C compiler's view of the same header: sizeof, every member's offsetof, every enumerator."""
import ctypes
import os
import shutil
import subprocess

import pytest

STRUCTS = ("ea_epilogue", "ea_conv_geo", "ea_group_gemm", "ea_colsum_prob", "ea_reduce_prob",
           "ea_lr_schedule", "ea_opt_state")


def test_generated_binding_matches_c_compiler(tmp_path):
    from espnet_amd import _lib
    cc = next((c for c in (os.environ.get("CC"), "cc", "gcc", "clang") if c and shutil.which(c)), None)
    if cc is None:
        pytest.skip("no C compiler")
    assert set(_lib.STRUCTS) == set(STRUCTS)
    lines = ["#include <stdio.h>", "#include <stddef.h>", '#include "espnet_amd.h"', "int main(void) {"]
    for name, cls in _lib.STRUCTS.items():
        lines.append(f'  printf("{name} %zu\\n", sizeof({name}));')
        for field, _ in cls._fields_:
            lines.append(f'  printf("{name}.{field} %zu\\n", offsetof({name}, {field}));')
    for name in _lib.ENUMS:
        lines.append(f'  printf("{name} %d\\n", (int){name});')
    lines += ["  return 0;", "}"]
    src = tmp_path / "abi.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "abi"
    subprocess.run([cc, "-I", os.path.dirname(_lib.HEADER), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    c_view = {k: int(v) for k, v in (line.split() for line in out.splitlines())}

    py_view = dict(_lib.ENUMS)
    for name, cls in _lib.STRUCTS.items():
        py_view[name] = ctypes.sizeof(cls)
        for field, _ in cls._fields_:
            py_view[f"{name}.{field}"] = getattr(cls, field).offset
    assert py_view == c_view
    # a struct whose last members the parser dropped would still match member by member
    assert len(_lib.ENUMS) >= 16 and all(len(c._fields_) >= 3 for c in _lib.STRUCTS.values())

    # the module-level names are the parsed values, and the classes the parsed classes
    for name, value in _lib.ENUMS.items():
        assert getattr(_lib, name[len("EA_"):]) == value
    assert _lib.Epilogue is _lib.STRUCTS["ea_epilogue"] and _lib.ConvGeo is _lib.STRUCTS["ea_conv_geo"]
    assert _lib.GroupGemm is _lib.STRUCTS["ea_group_gemm"] and _lib.LrSchedule is _lib.STRUCTS["ea_lr_schedule"]
    assert _lib.ColsumProb is _lib.STRUCTS["ea_colsum_prob"] and _lib.ReduceProb is _lib.STRUCTS["ea_reduce_prob"]
    assert _lib.OPT_STATE_BYTES == c_view["ea_opt_state"] == 40
    assert _lib.OPT_STATE_NEXT_LR * 4 == c_view["ea_opt_state.next_lr"]


def test_unknown_member_form_raises(tmp_path):
    from espnet_amd import _lib
    for member in ("short s;", "int (*fn)(int);", "int grid[2][2];", "struct ea_x* next, *prev;"):
        h = tmp_path / "bad.h"
        h.write_text("typedef struct ea_bad { int ok; %s } ea_bad;\n" % member)
        with pytest.raises(TypeError):
            _lib.parse_abi(str(h))
    h.write_text("enum { EA_A = 1, EA_B };\n")
    with pytest.raises(TypeError):
        _lib.parse_abi(str(h))


def test_switches_assigned_through_hip_ops_reach_their_home_module():
    """hip_ops.<switch> of a switch that lives in streams / deferred is that switch, not a copy."""
    from espnet_amd import deferred, hip_ops, streams
    for home, name, value in [(streams, "DEBUG_DELAY_NS", 123), (streams, "DEBUG_SERIAL", True),
                              (streams, "OVERLAP_CTC_BWD", False), (deferred, "GRAD_READY", print),
                              (deferred, "DEFER_WGRAD", False), (deferred, "DEFER_REDUCE", False),
                              (deferred, "DEFER_BUDGET", 1)]:
        prev = getattr(home, name)
        try:
            setattr(hip_ops, name, value)
            assert getattr(home, name) is value and getattr(hip_ops, name) is value
            assert name not in vars(hip_ops)
        finally:
            setattr(home, name, prev)
        assert getattr(hip_ops, name) is prev
    with pytest.raises(AttributeError):
        hip_ops.NO_SUCH_SWITCH
