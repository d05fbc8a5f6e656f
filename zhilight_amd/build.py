"""Build the gfx950 shared library (hipcc cross-compiles without a GPU).

    python -m zhilight_amd.build [--force]

Produces zhilight_amd/libzhilight_amd.so in-tree (git-ignored, but it travels with gpurun snapshots).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "libzhilight_amd.so")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
         "-fno-fast-math", "-ffp-contract=off"]
# per-source extras.  w4_slab.hip: its item loops (up to 4 groups x 8 tiles, the next group's normalisation in slices between the
# items) must unroll completely -- ring slots, accumulators and wait counts are static only then -- and the NORM instantiations
# exceed the unroller's default budget for `#pragma unroll` (16 K): the ring went to scratch behind dynamic indices
EXTRA_FLAGS = {"w4_slab.hip": ["-mllvm", "-pragma-unroll-threshold=200000"]}


# ZL_BUILD_EXPERIMENTAL=1: also build what was measured and left off the product path: the loader /
# consumer engine (tools/experimental/w4_engine.hip -- it is not in csrc/) and the digit-plane entry points for 5..32 rows (the
# #ifdef ZL_EXPERIMENTAL blocks of w4_phase.hip / w4_mfma.hip); their tests live next to the engine, tools/experimental/test_gpu_*.py
# (python -m pytest tools/experimental -m gpu, after such a build).  The default library and the default test run carry neither.
EXPERIMENTAL = os.environ.get("ZL_BUILD_EXPERIMENTAL", "0") == "1"
EXPERIMENTAL_DIR = os.path.join(HERE, "..", "tools", "experimental")


def sources():
    srcs = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))
    if EXPERIMENTAL:
        srcs.append(os.path.join(EXPERIMENTAL_DIR, "w4_engine.hip"))
    return srcs


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    srcs = sources()
    hdrs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    hdrs.append(os.path.join(HERE, "..", "include", "zhilight_amd.h"))
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    flags = FLAGS + (["-DZL_EXPERIMENTAL", "-I" + CSRC] if EXPERIMENTAL else [])
    stamp = os.path.join(objdir, ".flags")
    if not os.path.exists(stamp) or open(stamp).read() != " ".join(flags):
        force = True                                   # another flavour's objects: rebuild all of them
    objs = []
    jobs = []
    for s in srcs:
        o = os.path.join(objdir, os.path.basename(s)[:-4] + ".o")
        objs.append(o)
        if force or _stale(o, [s] + hdrs):
            jobs.append([HIPCC] + flags + EXTRA_FLAGS.get(os.path.basename(s), []) + ["-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(8, max(1, len(jobs)))) as ex:
        list(ex.map(run, jobs))
    if jobs or force or _stale(OUT, objs):
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs)
    with open(stamp, "w") as fh:
        fh.write(" ".join(flags))
    build_hostcpp(force, verbose)
    build_comm(force, verbose)
    _ref().build(force, verbose)
    return OUT


COMM_OUT = os.path.join(HERE, "libzhilight_amd_comm.so")


def build_comm(force=False, verbose=False):
    """libzhilight_amd_comm.so: the tensor-parallel exchange step (direct RCCL communicator + one-shot peer-read all-reduce,
    include/zhilight_amd_comm.h).  Separate from the main library so that single-GPU users carry no RCCL dependency."""
    src = os.path.join(HERE, "csrc_comm", "comm.hip")
    deps = [src, os.path.join(HERE, "..", "include", "zhilight_amd_comm.h"), os.path.join(HERE, "..", "include", "zhilight_amd.h")]
    if not (force or _stale(COMM_OUT, deps)):
        return COMM_OUT
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-shared", "-o", COMM_OUT, src,
           "-L" + os.path.join(rocm, "lib"), "-lrccl"]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return COMM_OUT


HOSTCPP = os.path.join(HERE, "hostcpp")


HOSTCPP_SOURCES = ("bm_hip.cpp", "bm_layer.cpp", "bm_functions.cpp", "bm_c10d.cpp", "nn_amd.cpp")
HOSTCPP_HEADERS = ("bm_hip.h", "bm_layer.h", "bm_functions.h", "bm_c10d.h", "nn_amd.h")


def hostcpp_target():
    import sysconfig
    return os.path.join(HERE, "zl_internals" + sysconfig.get_config_var("EXT_SUFFIX"))


def build_hostcpp(force=False, verbose=False):
    """The C++ host layer (bmengine-on-HIP shim + the reference's nn:: / int8_op:: operator names over the C ABI) and its
    pybind11 test module zhilight_amd/zl_internals*.so.  Host code only: g++ against the HIP runtime headers."""
    import pybind11
    import sysconfig
    srcs = [os.path.join(HOSTCPP, f) for f in HOSTCPP_SOURCES + ("py_internals.cpp",)]
    deps = srcs + [os.path.join(HOSTCPP, f) for f in HOSTCPP_HEADERS] + [os.path.join(HERE, "..", "include", "zhilight_amd.h")]
    target = hostcpp_target()
    if not (force or _stale(target, deps)):
        return target
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
           "-I" + os.path.join(HERE, "..", "include"), "-I" + pybind11.get_include(), "-I" + sysconfig.get_paths()["include"]] + srcs + [
           "-o", target, "-L" + HERE, "-lzhilight_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(rocm, "lib")]
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    return target


REFERENCE = os.environ.get("ZL_REFERENCE_ROOT", "/root/reference")
# the reference binaries (test infrastructure, never part of the package): the recipe is oracle/ref_build.py, its products go to
# oracle/_ref/ (git-ignored).  Its names stay reachable here: build.REF_TUS, build.refcompile_target(), build.build_binding(), ...
ORACLE = os.path.join(os.path.dirname(HERE), "oracle")
_REF_NAMES = ("REFDIR", "REF_TUS", "REF_CHECK_TUS", "REF_CHECK_NAMESPACES", "REF_REPORT_TUS", "REF_CHECK_PENDING",
              "REF_BINDING_TUS", "HOST_SOURCES", "HOST_HEADERS", "HARNESS_SOURCES", "host_target", "refcompile_target",
              "binding_target", "refcheck_report", "build_host", "build_refcompile", "build_binding", "build_refcheck")


def _ref():
    if ORACLE not in sys.path:
        sys.path.insert(0, ORACLE)
    import ref_build
    return ref_build


def __getattr__(name):
    if name in _REF_NAMES:
        return getattr(_ref(), name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
