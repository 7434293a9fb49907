"""The native launch module (csrc/dispatch: entry points templated over csrc/kernels/pa_api.h, ops/_sigs.py checked
against it at build): the table against the exports, argument conversion and parity with the ctypes path on
launchers that do not touch the GPU."""
import ctypes
import importlib.util
import os
import subprocess

import numpy as np
import pytest
import torch

from paddlepaddle_amd.ops import _loader as L
from paddlepaddle_amd.ops import _sigs

D = pytest.importorskip("paddlepaddle_amd._C_dispatch")


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _build_native():
    spec = importlib.util.spec_from_file_location("_build_native", os.path.join(ROOT, "tools", "build_native.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_every_exported_launcher_has_an_entry_point():
    """The launchers _C_hip.so exports are exactly the rows of the table, and each has a native entry point."""
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "paddlepaddle_amd", "_C_hip.so")],
                        capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in nm.splitlines() if ln.strip()}
    exported = {n for n in exported if n.startswith("pa_")}
    assert exported
    assert exported - set(_sigs.SIGS) == set(), "exported without a row in ops/_sigs.py"
    assert set(_sigs.SIGS) - exported == set(), "rows in ops/_sigs.py that no kernel defines"
    assert [n for n in sorted(exported) if not hasattr(D, n)] == []


def test_tracked_dispatch_table_is_current():
    b = _build_native()
    with open(b.DISPATCH_GEN) as f:
        assert f.read() == b.dispatch_gen_text()


_SIG_SNIPPET = """
#include "pa_api.h"
#include "sig_code.h"
static_assert(pa_sig::sig(&pa_rms_norm_fwd) == "%s", "ops/_sigs.py disagrees with pa_api.h: pa_rms_norm_fwd");
"""


@pytest.mark.parametrize("code,ok", [("ippppllfip", True), ("ipppplifip", False), ("lppppllfip", False)],
                         ids=["right", "wrong-argument", "wrong-return"])
def test_signature_check_bites(code, ok):
    """The compile-time check of dispatch.cpp, on its own: the code of pa_rms_norm_fwd passes, one changed argument
    letter or a changed return letter fails with the launcher's name in the diagnostic."""
    b = _build_native()
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__=1", f"-I{b.ROCM}/include",
                        f"-I{b.KERNELS}", "-I" + os.path.join(ROOT, "csrc", "dispatch"), "-x", "c++", "-"],
                       input=_SIG_SNIPPET % code, capture_output=True, text=True)
    if ok:
        assert r.returncode == 0, r.stderr
    else:
        assert r.returncode != 0 and "static assertion failed" in r.stderr and "pa_rms_norm_fwd" in r.stderr


def test_host_only_launchers_match_ctypes():
    lib = L.lib()
    for R, C in ((1024, 64), (802816, 256), (3136, 2048)):
        assert D.pa_bn_chunks(R, C) == lib.pa_bn_chunks(R, C)
        assert D.pa_bn_chunks(np.int64(R), ctypes.c_int(C)) == lib.pa_bn_chunks(R, C)  # numpy / ctypes scalars
    old = D.pa_bn_set_target_wgs(777)
    assert lib.pa_bn_set_target_wgs(old) == 777
    assert D.pa_version() == lib.pa_version()


def test_argument_errors_are_python_exceptions():
    with pytest.raises(TypeError, match="takes 9 arguments"):
        D.pa_rms_norm_fwd(1, 2)
    with pytest.raises(TypeError, match="pointer"):
        D.pa_rms_norm_fwd("x", None, None, None, 1, 1, 1.0, 0, L.CURRENT_STREAM)
    with pytest.raises(TypeError):
        D.pa_bn_chunks(1.5j, 3)


def test_loader_hands_objects_through_on_the_native_path():
    if not L.native_launch():
        pytest.skip("PADDLE_AMD_CTYPES_LAUNCH=1")
    t = torch.zeros(3)
    assert L.ptr(t) is t and L.ptr(None) is None
    assert L.stream_ptr() is L.CURRENT_STREAM
    assert os.environ.get("PADDLE_AMD_CTYPES_LAUNCH", "0") != "1"
