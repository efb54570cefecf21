"""h264bsdmiNextOutputTensorBatch without a GPU: the ABI (symbol, descriptor layout) and the checks that refuse a call before
anything is popped."""
import ctypes
import os
import re
import subprocess

import pytest

from conftest import ROOT, stream_bytes

SYMBOL = "h264bsdmiNextOutputTensorBatch"


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {line.split()[-1] for line in out.splitlines() if " T " in line}


def test_symbol_is_declared_exported_and_mirrored(built):
    text = open(os.path.join(ROOT, "include", "h264bsd_mi355x.h")).read()
    assert re.search(r"\bint\s+" + SYMBOL + r"\s*\(", text)
    assert SYMBOL in built.EXPORTED_SYMBOLS
    built.lib()
    assert SYMBOL in _exported(built.LIB_PATH)
    assert SYMBOL in _exported(built.capi.BENCH_LIB_PATH)


def test_tensor_spec_layout_matches_the_ctypes_mirror(built, tmp_path):
    fields = [f[0] for f in built.TensorSpec._fields_]
    src = tmp_path / "spec.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "h264bsd_mi355x.h"\nint main(void) {\n'
                   '    printf("%zu\\n", sizeof(h264bsdmi_tensor_spec));\n' +
                   "".join(f'    printf("%zu\\n", offsetof(h264bsdmi_tensor_spec, {f}));\n' for f in fields) + "    return 0;\n}\n")
    exe = tmp_path / "spec"
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = [ctypes.sizeof(built.TensorSpec)] + [getattr(built.TensorSpec, f).offset for f in fields]
    assert got == want


def _spec(built, **kw):
    s = dict(data=0x1000, width=640, height=360, layout=0, dtype=1, channels=0, crop=1, resize=0, mean=(0, 0, 0), std=(1, 1, 1))
    s.update(kw)
    return built.TensorSpec(s["data"], s["width"], s["height"], s["layout"], s["dtype"], s["channels"], s["crop"], s["resize"],
                            (ctypes.c_float * 3)(*s["mean"]), (ctypes.c_float * 3)(*s["std"]))


def _call(built, decoders, spec):
    L = built.api_lib()
    n = len(decoders)
    got = (ctypes.c_uint32 * max(n, 1))()
    dec = (ctypes.c_void_p * max(n, 1))(*[d._st for d in decoders])
    return L.h264bsdmiNextOutputTensorBatch(n, dec, ctypes.byref(spec), None, got, None, None, None)


@pytest.mark.parametrize("bad", [
    dict(data=0), dict(width=0), dict(height=0), dict(layout=2), dict(dtype=3), dict(channels=5),
    dict(layout=0, channels=2), dict(layout=0, channels=3), dict(dtype=0, mean=(0.5, 0, 0)), dict(dtype=0, std=(1, 2, 1)),
    dict(std=(1, 0, 1)),
])
def test_invalid_specs_are_refused(built, bad):
    """checked before any instance is looked at: an empty batch with a bad spec fails, one with a good spec succeeds"""
    assert _call(built, [], _spec(built)) == 0
    assert _call(built, [], _spec(built, **bad)) < 0


def test_nhwc_four_channels_and_normalised_floats_are_accepted(built):
    assert _call(built, [], _spec(built, layout=1, channels=2)) == 0
    assert _call(built, [], _spec(built, dtype=2, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))) == 0


def _capture_until_output(built):
    """a parser-only instance fed up to its first picture in the output queue"""
    data = stream_bytes("test_640x360")
    dec = built.Decoder(capture=lambda blob: None)
    buf = ctypes.create_string_buffer(data, len(data))
    off = 0
    while off < len(data):
        r, rb = dec.decode(ctypes.addressof(buf) + off, len(data) - off)
        off += rb
        if r == built.H264BSD_PIC_RDY:
            break
    return dec, buf


def test_capture_mode_instance_is_refused_and_keeps_its_picture(built):
    a, keep_a = _capture_until_output(built)
    b, keep_b = _capture_until_output(built)
    assert _call(built, [a], _spec(built)) < 0
    assert _call(built, [a], _spec(built, resize=1, width=224, height=224)) < 0
    info = a.next_output_info()
    assert info is not None and info == b.next_output_info()
    a.close()
    b.close()

