#!/usr/bin/env python3
"""Build the native parts of paddlepaddle_amd in-tree.

* ``paddlepaddle_amd/_C_hip.so``     — every csrc/kernels/*.hip, hipcc --offload-arch=gfx950, C ABI
                                        (loaded with ctypes by paddlepaddle_amd.ops._loader)
* ``paddlepaddle_amd/_C_runtime*.so`` — csrc/runtime/*.cpp, g++ + pybind11 (CPU runtime)
* ``paddlepaddle_amd/_C_dispatch*.so`` — csrc/dispatch/dispatch.cpp: the native launch path of every ``pa_*``
                                        launcher, one template instantiation per declaration in
                                        csrc/kernels/pa_api.h (links _C_hip.so, libtorch). dispatch_gen.inc, generated
                                        from the ctypes table ops/_sigs.py, is the list of launchers and the check
                                        that the table agrees with pa_api.h: a disagreement fails this build.

Incremental: an object is rebuilt only when its source or a header of csrc/kernels is newer; the C++ callers of the
kernels also when pa_api.h is. Parallel compile.
"""
from __future__ import annotations

import concurrent.futures as cf
import glob
import os
import subprocess
import sys
import sysconfig

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
BUILD = os.path.join(ROOT, "build", "native")
PKG = os.path.join(ROOT, "paddlepaddle_amd")
KERNELS = os.path.join(ROOT, "csrc", "kernels")
PA_API = os.path.join(KERNELS, "pa_api.h")  # the C API of _C_hip.so, included by every C++ caller of the kernels

HIP_FLAGS = ["-O3", "-std=c++17", "-fPIC", f"--offload-arch={ARCH}", "-munsafe-fp-atomics",
             "-Wno-unused-result", "-Wno-unused-variable"]


def _newer(src_list, out):
    if not os.path.exists(out):
        return True
    t = os.path.getmtime(out)
    return any(os.path.getmtime(s) > t for s in src_list)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + r.stderr)
        raise SystemExit(f"build failed: {cmd[-1] if cmd else ''}")
    return r


def build_hip(verbose=False, jobs=None):
    srcs = sorted(glob.glob(os.path.join(ROOT, "csrc", "kernels", "*.hip")))
    hdrs = glob.glob(os.path.join(ROOT, "csrc", "kernels", "*.h"))
    os.makedirs(BUILD, exist_ok=True)
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    objs = []
    todo = []
    for s in srcs:
        o = os.path.join(BUILD, os.path.basename(s) + ".o")
        objs.append(o)
        if _newer([s] + hdrs, o):
            todo.append((s, o))
    jobs = jobs or min(8, max(1, os.cpu_count() or 1))
    with cf.ThreadPoolExecutor(jobs) as ex:
        futs = [ex.submit(_run, [hipcc, *HIP_FLAGS, "-c", s, "-o", o]) for s, o in todo]
        for f in futs:
            f.result()
    out = os.path.join(PKG, "_C_hip.so")
    if todo or _newer(objs, out):
        _run([hipcc, "-shared", "-fPIC", f"--offload-arch={ARCH}", "-o", out, *objs, f"-L{ROCM}/lib", "-lamdhip64"])
    if verbose:
        print(f"built {out} ({len(todo)} objects recompiled)")
    return out


def build_runtime(verbose=False):
    import pybind11
    srcs = sorted(s for s in glob.glob(os.path.join(ROOT, "csrc", "runtime", "*.cpp")) if not s.endswith("_hip.cpp"))
    hdrs = glob.glob(os.path.join(ROOT, "csrc", "runtime", "*.h"))
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    out = os.path.join(PKG, "_C_runtime" + suffix)
    if not _newer(srcs + hdrs, out):
        return out
    inc = [f"-I{pybind11.get_include()}", f"-I{sysconfig.get_paths()['include']}"]
    _run(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", *inc, *srcs, "-o", out, "-ldl"])
    if verbose:
        print(f"built {out}")
    return out


def build_alloc(verbose=False):
    """The HIP device allocator (host code, hipMalloc / events) as a PyTorch pluggable allocator library."""
    srcs = sorted(glob.glob(os.path.join(ROOT, "csrc", "runtime", "*_hip.cpp")))
    hdrs = glob.glob(os.path.join(ROOT, "csrc", "runtime", "*.h"))
    out = os.path.join(PKG, "_C_alloc.so")
    if not _newer(srcs + hdrs, out):
        return out
    hipcc = os.path.join(ROCM, "bin", "hipcc")
    _run([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", *srcs, "-o", out, f"-L{ROCM}/lib", "-lamdhip64"])
    if verbose:
        print(f"built {out}")
    return out


_CTYPE_TO_CODE = {"c_void_p": "p", "c_long": "l", "c_longlong": "l", "c_int": "i", "c_float": "f", "c_ulong": "u",
                  "c_ulonglong": "u"}


def _load_sigs():
    import importlib.util
    spec = importlib.util.spec_from_file_location("_pa_sigs", os.path.join(PKG, "ops", "_sigs.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def dispatch_gen_text():
    """The text of csrc/dispatch/dispatch_gen.inc: one ``PA_ENTRY(name, code)`` row per launcher in ops/_sigs.py,
    the code being the return type's letter then one per argument (csrc/dispatch/sig_code.h). dispatch.cpp
    static_asserts each code against the declaration in csrc/kernels/pa_api.h, so a row that is wrong, or that has
    no declaration, stops the build."""
    m = _load_sigs()
    out = ["// generated by tools/build_native.py from paddlepaddle_amd/ops/_sigs.py -- do not edit"]
    for name, args in m.SIGS.items():
        code = ("l" if name in m.RET_I64 else "i") + "".join(_CTYPE_TO_CODE[a.__name__] for a in args)
        out.append(f'PA_ENTRY({name}, "{code}")')
    return "\n".join(out) + "\n"


DISPATCH_GEN = os.path.join(ROOT, "csrc", "dispatch", "dispatch_gen.inc")


def gen_dispatch():
    text = dispatch_gen_text()
    if not os.path.exists(DISPATCH_GEN) or open(DISPATCH_GEN).read() != text:
        with open(DISPATCH_GEN, "w") as f:
            f.write(text)
    return DISPATCH_GEN


def build_dispatch(verbose=False):
    import torch.utils.cpp_extension as ce
    gen = gen_dispatch()
    src = os.path.join(ROOT, "csrc", "dispatch", "dispatch.cpp")
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    out = os.path.join(PKG, "_C_dispatch" + suffix)
    hip_so = os.path.join(PKG, "_C_hip.so")
    if not _newer([src, gen, os.path.join(ROOT, "csrc", "dispatch", "sig_code.h"), PA_API, hip_so], out):
        return out
    inc = [f"-I{d}" for d in ce.include_paths()] + [f"-I{sysconfig.get_paths()['include']}", f"-I{ROCM}/include",
                                                     f"-I{KERNELS}"]
    libs = [f"-L{d}" for d in ce.library_paths()] + [ "-ltorch_python", "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip",
            f"-L{PKG}", "-l:_C_hip.so", f"-L{ROCM}/lib", "-lamdhip64", "-Wl,-rpath,$ORIGIN"]
    _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
          "-D_GLIBCXX_USE_CXX11_ABI=1", *inc, src, "-o", out, *libs])
    if verbose:
        print(f"built {out}")
    return out


def build_interp(verbose=False):
    """``_C_interp``: the native program interpreter (csrc/interpreter/interpreter.cpp) — a torch C++ extension
    (pybind11 + ATen) that launches the hand-written kernels of _C_hip.so (no device code of its own)."""
    import torch.utils.cpp_extension as ce
    src = os.path.join(ROOT, "csrc", "interpreter", "interpreter.cpp")
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    out = os.path.join(PKG, "_C_interp" + suffix)
    hip_so = os.path.join(PKG, "_C_hip.so")
    if not _newer([src, PA_API, hip_so], out):
        return out
    inc = [f"-I{d}" for d in ce.include_paths()] + [f"-I{sysconfig.get_paths()['include']}", f"-I{ROCM}/include",
                                                     f"-I{KERNELS}"]
    # links the hand-written kernels (_C_hip.so) and c10_hip (current HIP stream), like _C_dispatch
    libs = [f"-L{d}" for d in ce.library_paths()] + ["-ltorch_python", "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip",
                                                      f"-L{PKG}", "-l:_C_hip.so", f"-L{ROCM}/lib", "-lamdhip64",
                                                      "-Wl,-rpath,$ORIGIN"]
    _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
          "-D_GLIBCXX_USE_CXX11_ABI=1", "-DTORCH_EXTENSION_NAME=_C_interp", "-DTORCH_API_INCLUDE_EXTENSION_H", *inc,
          src, "-o", out, *libs])
    if verbose:
        print(f"built {out}")
    return out


def build_train(verbose=False):
    """``_C_train``: the native training executor (csrc/interpreter/train_interp.cpp) — forward instructions on the
    hand-written kernels / ATen dispatcher, C++ autograd backward, fused optimizer kernels (_C_hip.so)."""
    import torch.utils.cpp_extension as ce
    src = os.path.join(ROOT, "csrc", "interpreter", "train_interp.cpp")
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    out = os.path.join(PKG, "_C_train" + suffix)
    hip_so = os.path.join(PKG, "_C_hip.so")
    if not _newer([src, PA_API, hip_so], out):
        return out
    inc = [f"-I{d}" for d in ce.include_paths()] + [f"-I{sysconfig.get_paths()['include']}", f"-I{ROCM}/include",
                                                     f"-I{KERNELS}"]
    libs = [f"-L{d}" for d in ce.library_paths()] + ["-ltorch_python", "-ltorch", "-ltorch_cpu", "-lc10", "-lc10_hip",
                                                      f"-L{PKG}", "-l:_C_hip.so", f"-L{ROCM}/lib", "-lamdhip64",
                                                      "-Wl,-rpath,$ORIGIN"]
    _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
          "-D_GLIBCXX_USE_CXX11_ABI=1", "-DTORCH_EXTENSION_NAME=_C_train", "-DTORCH_API_INCLUDE_EXTENSION_H", *inc,
          src, "-o", out, *libs])
    if verbose:
        print(f"built {out}")
    return out


def build_autograd(verbose=False):
    """``_C_autograd``: the native backward executor (csrc/autograd/autograd_exec.cpp) — torch C++ extension over
    the autograd Node interface (pybind11 + libtorch)."""
    import torch.utils.cpp_extension as ce
    src = os.path.join(ROOT, "csrc", "autograd", "autograd_exec.cpp")
    suffix = sysconfig.get_config_var("EXT_SUFFIX") or ".so"
    out = os.path.join(PKG, "_C_autograd" + suffix)
    if not _newer([src], out):
        return out
    inc = [f"-I{d}" for d in ce.include_paths()] + [f"-I{sysconfig.get_paths()['include']}", f"-I{ROCM}/include"]
    libs = [f"-L{d}" for d in ce.library_paths()] + ["-ltorch_python", "-ltorch", "-ltorch_cpu", "-lc10",
                                                      "-Wl,-rpath,$ORIGIN"]
    _run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1",
          "-D_GLIBCXX_USE_CXX11_ABI=1", "-DTORCH_EXTENSION_NAME=_C_autograd", "-DTORCH_API_INCLUDE_EXTENSION_H", *inc,
          src, "-o", out, *libs])
    if verbose:
        print(f"built {out}")
    return out


def main():
    verbose = "-v" in sys.argv or True
    build_hip(verbose)
    build_runtime(verbose)
    build_alloc(verbose)
    build_dispatch(verbose)
    build_interp(verbose)
    build_autograd(verbose)
    build_train(verbose)


if __name__ == "__main__":
    main()
