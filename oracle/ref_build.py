"""The reference binaries: test infrastructure, never part of the package.

    python oracle/ref_build.py [--force]

Compiles the reference's host translation units UNMODIFIED, read in place from the reference tree (ZL_REFERENCE_ROOT), against
this repository's boundary (zhilight_amd/hostcpp: the bmengine-on-HIP layer, refshim and the pybind11 harness) into oracle/_ref/
(git-ignored): libzhilight_amd_host.so, the test module zl_reflinear*.so, the reference's own `zhilight.C` (C*.so) and the link
report linkcheck.json.  Nothing of the reference is copied; without the tree, the prebuilt files in oracle/_ref/ are used as they
are.  zhilight_amd.build.build() runs this recipe after the package library, and re-exports its names.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ORACLE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(ORACLE)
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from zhilight_amd import build as zb  # noqa: E402  (the package library, its sources and staleness rule)

PKG = zb.HERE
HOSTCPP = zb.HOSTCPP
INCLUDE = os.path.join(ROOT, "include")
REFERENCE = zb.REFERENCE
REFDIR = os.path.join(ORACLE, "_ref")
# reference host translation units compiled UNMODIFIED, from where they lie, against hostcpp/refshim + the bmengine-on-HIP
# headers ("prove the boundary compiles the reference")
REF_TUS = ("src/nn/linear/linear.cpp", "src/nn/attention/attention.cpp", "src/nn/attention/multi_head_latent_attention.cpp",
           "src/nn/feedforward/feedforward.cpp", "src/nn/block/block.cpp", "src/model/llama.cpp", "src/model/model_context.cpp",
           "src/model/buffer_context.cpp", "src/kvcache/block_allocator.cpp", "src/model/host_all_reducer.cpp")
# reference translation units that are compiled unmodified and LINK-CHECKED only (build_refcheck): every name they reference in the
# namespaces the boundary stands in for must be defined by the boundary under the same mangled name -- i.e. with the reference's
# exact signature; names of layers that are not on the path (their device code lives in the reference's .cu files) are listed
REF_CHECK_TUS = ("src/nn/attention/attention.cpp", "src/nn/attention/multi_head_latent_attention.cpp", "src/nn/feedforward/feedforward.cpp",
                 "src/nn/block/block.cpp", "src/model/llama.cpp", "src/model/model_context.cpp", "src/model/buffer_context.cpp")
REF_CHECK_NAMESPACES = ("ds::", "bmengine::", "nn::fp8::", "nn::gptq::", "int8_op::", "nn::top_k_softmax(", "nn::group_topk_softmax(",
                        "nn::sum_experts(", "nn::route_shared_lb(", "nn::plus_for_sort(", "nn::calc_reverse_idx(",
                        "nn::fill_m_indices_padded_indices(", "nn::gate_mul_inplace(", "nn::gate_fuse(", "nn::gelu_inplace(", "nn::silu_inplace(",
                        "nn::attention_qkv_rag_buffer(", "nn::multi_query_attention_rag_buffer(", "nn::get_mqa_workspace(", "nn::rope_qk_cache(",
                        "nn::rotary_embedding_qk(", "nn::copy_to_rag_buffer2(")
# attempted and REPORTED only (never fail the build): what a full drop-in of zhilight.C would still need
REF_REPORT_TUS = ("src/py_export/bind.cpp", "src/py_export/py_batch_generator.cpp", "src/py_export/py_llama.cpp", "src/py_export/py_model_base.cpp",
                  "src/py_export/py_model_config.cpp", "src/py_export/py_utils.cpp", "src/generator/batch_generator.cpp")
# declared by the shim so that the units compile, NOT provided by the boundary (smooth-quant calibration helpers): reported as "pending"
# (round 4: the MoE dispatch route's arange / sort_pair_1d / divide / scatter_update_dim0 left this list -- bm_functions.cpp)
REF_CHECK_PENDING = ("bmengine::functions::pow(", "bmengine::functions::clamp(")


# the host library: the bmengine-on-HIP layer, the engine, the classes around the operators (host_*.cpp) and the reference's units
HOST_SOURCES = zb.HOSTCPP_SOURCES + ("bm_engine.cpp", "host_kvcache.cpp", "host_position.cpp", "host_embedding.cpp", "host_layernorm.cpp",
                                  "host_attention_ext.cpp", "host_offpath.cpp", "host_generator_ext.cpp")
HOST_HEADERS = zb.HOSTCPP_HEADERS + ("bm_engine.h", "host_common.h")
# the pybind11 harness around it (test infrastructure)
HARNESS_SOURCES = (os.path.join("refshim", "ref_glue.cpp"), "ref_attention_glue.cpp", "ref_block_glue.cpp", "ref_model_glue.cpp")


def host_target():
    return os.path.join(REFDIR, "libzhilight_amd_host.so")


def refcompile_target():
    import sysconfig
    return os.path.join(REFDIR, "zl_reflinear" + sysconfig.get_config_var("EXT_SUFFIX"))


def _ref_compile_env():
    import pybind11
    import sysconfig
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    shim = os.path.join(HOSTCPP, "refshim")
    inc = ["-I" + shim, "-I" + HOSTCPP, "-I" + os.path.join(rocm, "include"), "-I" + INCLUDE,
           "-I" + os.path.join(REFERENCE, "src"), "-I" + REFERENCE, "-I" + pybind11.get_include(), "-I" + sysconfig.get_paths()["include"]]
    cxx = os.environ.get("CXX", "g++")
    return rocm, shim, cxx, [cxx, "-O1", "-std=c++17", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-DENABLE_DS_DEEP_GEMM", "-DZL_REF_LAYERNORM_EXTERNAL", "-w"] + inc


def _undefined_outside(target, libs):
    """names `target` needs that none of `libs` defines (the CPython API and the C / C++ runtime aside)"""
    have = set()
    for lib in libs:
        for line in subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines():
            have.add(line.split()[-1])
    missing = []
    for line in subprocess.check_output(["nm", "-D", "-u", target], text=True).splitlines():
        kind, sym = line.split()[-2:]
        if kind in "wv" or "@" in sym or sym.startswith(("Py", "_Py", "__")) or sym in have:
            continue
        missing.append(sym)
    return missing


def build_host(force=False, verbose=False):
    """oracle/_ref/libzhilight_amd_host.so = the host library a drop-in of the reference links instead of its .cu files and
    bmengine: the bmengine-on-HIP layer (Context / Tensor / Layer / functions / c10d), core::Engine (one thread + one exchange state +
    one RCCL communicator per tensor-parallel rank, bm_engine.cpp), the operator wrappers under the reference's names (nn_amd.cpp), the
    classes around them (host_*.cpp: TransformerBuffer, RotaryEmbedding, RopePreparer, RawEmbedding incl. its vocab-parallel form,
    the reference-layout LayerNorm, FlashDecoding::mha_fwd) -- and, compiled UNMODIFIED from where they lie in the reference tree,
    the reference's own host translation units REF_TUS (linear, attention, MLA, feed-forward, block, llama, model_context,
    buffer_context).  Links libzhilight_amd.so and libzhilight_amd_comm.so.  Only where the reference tree exists; a
    machine without it uses the prebuilt file.  oracle/_ref/ is git-ignored (it holds compiled reference code) and travels with
    the built tree.  Returns the path, or None without a reference."""
    target = host_target()
    if target in _HOST_BUILT:                           # once per process: build_refcompile and build_binding both ask (a
        return _HOST_BUILT[target]                      # forced build compiled every reference unit twice)
    _HOST_BUILT[target] = _build_host(force, verbose)
    return _HOST_BUILT[target]


_HOST_BUILT = {}


def _build_host(force, verbose):
    target = host_target()
    tus = [os.path.join(REFERENCE, t) for t in REF_TUS]
    if not all(os.path.exists(t) for t in tus):
        return target if os.path.exists(target) else None
    rocm, shim, cxx, common = _ref_compile_env()
    own = [os.path.join(HOSTCPP, f) for f in HOST_SOURCES]
    deps = tus + own + [os.path.join(HOSTCPP, f) for f in HOST_HEADERS] + [os.path.join(INCLUDE, "zhilight_amd.h"),
                                                                            os.path.join(INCLUDE, "zhilight_amd_comm.h"), zb.OUT, zb.COMM_OUT]
    for root, _, files in os.walk(shim):
        deps += [os.path.join(root, f) for f in files if f != "ref_glue.cpp"]
    if not (force or zb._stale(target, deps)):
        return target
    os.makedirs(REFDIR, exist_ok=True)
    objs = []
    jobs = []
    for src in tus + own:
        o = os.path.join(REFDIR, os.path.basename(src).rsplit(".", 1)[0] + ".o")
        objs.append(o)
        jobs.append(common + ["-c", src, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(16, len(jobs))) as ex:
        list(ex.map(run, jobs))
    run([cxx, "-shared", "-o", target] + objs + ["-L" + PKG, "-lzhilight_amd", "-lzhilight_amd_comm", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lpthread",
                                                   "-Wl,-rpath,$ORIGIN/../../zhilight_amd", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    for o in objs:
        os.remove(o)
    # every name the reference's translation units need must be DEFINED by the boundary: a leftover undefined symbol would only
    # surface as an ImportError on the GPU machine
    missing = _undefined_outside(target, [zb.OUT, zb.COMM_OUT, os.path.join(rocm, "lib", "libamdhip64.so")])
    if missing:
        os.remove(target)
        demangled = subprocess.run(["c++filt"], input="\n".join(missing), text=True, capture_output=True).stdout
        raise RuntimeError("the reference translation units need names the boundary does not define:\n" + demangled)
    return target


def build_refcompile(force=False, verbose=False):
    """oracle/_ref/zl_reflinear*.so = the pybind11 TEST module around libzhilight_amd_host.so (HARNESS_SOURCES: RefLinear,
    RefAttention, RefEncoderLayer, RefFeedForward, RefLLaMA, RefEngineLLaMA).  Returns the path, or None without a reference."""
    target = refcompile_target()
    host = build_host(force, verbose)
    if host is None or not os.path.exists(REFERENCE):
        return target if os.path.exists(target) and host is not None else None
    rocm, shim, cxx, common = _ref_compile_env()
    srcs = [os.path.join(HOSTCPP, f) for f in HARNESS_SOURCES]
    if not (force or zb._stale(target, srcs + [host])):
        return target
    objs = []
    jobs = []
    for src in srcs:
        o = os.path.join(REFDIR, "harness_" + os.path.basename(src).rsplit(".", 1)[0] + ".o")
        objs.append(o)
        jobs.append(common + ["-c", src, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        list(ex.map(run, jobs))
    run([cxx, "-shared", "-o", target] + objs + ["-L" + REFDIR, "-lzhilight_amd_host", "-L" + PKG, "-lzhilight_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                                                   "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../../zhilight_amd", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    for o in objs:
        os.remove(o)
    missing = _undefined_outside(target, [host, zb.OUT, os.path.join(rocm, "lib", "libamdhip64.so")])
    if missing:
        os.remove(target)
        demangled = subprocess.run(["c++filt"], input="\n".join(missing), text=True, capture_output=True).stdout
        raise RuntimeError("the test module needs names the host library does not define:\n" + demangled)
    return target


# the reference's Python binding and dynamic-batch scheduler, compiled UNMODIFIED: together with libzhilight_amd_host.so they ARE zhilight.C
REF_BINDING_TUS = ("src/py_export/bind.cpp", "src/py_export/py_batch_generator.cpp", "src/py_export/py_llama.cpp", "src/py_export/py_model_base.cpp",
                   "src/py_export/py_model_config.cpp", "src/py_export/py_utils.cpp", "src/generator/batch_generator.cpp")


def binding_target():
    import sysconfig
    return os.path.join(REFDIR, "C" + sysconfig.get_config_var("EXT_SUFFIX"))


def build_binding(force=False, verbose=False):
    """oracle/_ref/C*.so = the reference's own `zhilight.C` extension module: src/py_export/*.cpp (the pybind11 surface zhilight.llama /
    zhilight.dynamic_batch import) and src/generator/batch_generator.cpp (the dynamic-batch scheduler: task queue, chunked prefill, beam /
    greedy / random search), every unit compiled unmodified from where it lies, linked against libzhilight_amd_host.so -- no unit of this
    repository is compiled into it.  Fails on a leftover undefined symbol.  Returns the path, or None without a reference."""
    target = binding_target()
    host = build_host(force, verbose)
    tus = [os.path.join(REFERENCE, t) for t in REF_BINDING_TUS]
    if host is None or not all(os.path.exists(t) for t in tus):
        return target if os.path.exists(target) and host is not None else None
    rocm, shim, cxx, common = _ref_compile_env()
    deps = tus + [host]
    for root, _, files in os.walk(shim):
        deps += [os.path.join(root, f) for f in files if f != "ref_glue.cpp"]
    if not (force or zb._stale(target, deps)):
        return target
    objs, jobs = [], []
    for src in tus:
        o = os.path.join(REFDIR, "binding_" + os.path.basename(src).rsplit(".", 1)[0] + ".o")
        objs.append(o)
        jobs.append(common + ["-c", src, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=len(jobs)) as ex:
        list(ex.map(run, jobs))
    run([cxx, "-shared", "-o", target] + objs + ["-L" + REFDIR, "-lzhilight_amd_host", "-L" + PKG, "-lzhilight_amd", "-L" + os.path.join(rocm, "lib"), "-lamdhip64",
                                                   "-lpthread", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath,$ORIGIN/../../zhilight_amd", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    for o in objs:
        os.remove(o)
    missing = _undefined_outside(target, [host, zb.OUT, os.path.join(rocm, "lib", "libamdhip64.so")])
    if missing:
        os.remove(target)
        demangled = subprocess.run(["c++filt"], input="\n".join(missing), text=True, capture_output=True).stdout
        raise RuntimeError("zhilight.C needs names the host library does not define:\n" + demangled)
    return target


def refcheck_report():
    return os.path.join(REFDIR, "linkcheck.json")


def build_refcheck(force=False, verbose=False):
    """Compile REF_CHECK_TUS in place against hostcpp/refshim and compare what they reference with what the boundary defines
    (libzhilight_amd.so + libzhilight_amd_host.so).  Writes oracle/_ref/linkcheck.json:
    {tu: {"resolved": [...], "outside": [...], "pending": [...], "reference": [... defined by another checked unit]}} (demangled); raises when a name in REF_CHECK_NAMESPACES is not
    defined -- a signature that drifted from the reference's -- unless it is one of REF_CHECK_PENDING.  Only where the reference tree exists; returns the report path or None."""
    import json
    import pybind11
    import sysconfig
    report = refcheck_report()
    tus = [os.path.join(REFERENCE, t) for t in REF_CHECK_TUS]
    module = build_refcompile(verbose=verbose)
    if module is None or not all(os.path.exists(t) for t in tus):
        return report if os.path.exists(report) else None
    shim = os.path.join(HOSTCPP, "refshim")
    deps = tus + [module, os.path.abspath(__file__)]
    for root, _, files in os.walk(shim):
        deps += [os.path.join(root, f) for f in files]
    if not (force or zb._stale(report, deps)):
        return report
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    inc = ["-I" + shim, "-I" + HOSTCPP, "-I" + os.path.join(rocm, "include"), "-I" + INCLUDE,
           "-I" + os.path.join(REFERENCE, "src"), "-I" + REFERENCE, "-I" + pybind11.get_include(), "-I" + sysconfig.get_paths()["include"]]
    common = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-fPIC", "-D__HIP_PLATFORM_AMD__", "-DENABLE_DS_DEEP_GEMM", "-w"] + inc
    have = set()
    for lib in (zb.OUT, host_target(), os.path.join(rocm, "lib", "libamdhip64.so")):
        for line in subprocess.check_output(["nm", "-D", "--defined-only", lib], text=True).splitlines():
            have.add(line.split()[-1])
    out, drifted = {}, []
    objs = [os.path.join(REFDIR, os.path.basename(src).rsplit(".", 1)[0] + ".check.o") for src in tus]

    def compile_one(job):
        src, obj = job
        cmd = common + ["-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=len(tus)) as ex:
        list(ex.map(compile_one, zip(tus, objs)))
    undefined, other_units = {}, set()               # names one checked unit needs and another one defines are the reference's own
    for obj in objs:
        undefined[obj] = [line.split()[-1] for line in subprocess.check_output(["nm", "-u", obj], text=True).splitlines()]
        for line in subprocess.check_output(["nm", "--defined-only", obj], text=True).splitlines():
            other_units.add(line.split()[-1])
        os.remove(obj)
    for rel, obj in zip(REF_CHECK_TUS, objs):
        syms = undefined[obj]
        names = subprocess.run(["c++filt"], input="\n".join(syms), text=True, capture_output=True).stdout.splitlines()
        resolved, outside, pending, reference = [], [], [], []
        for sym, name in zip(syms, names):
            if sym == name:                                       # C symbols: libc / libm / the HIP runtime (versioned there)
                continue
            if name.startswith(("std::", "operator ", "vtable for", "typeinfo for", "VTT for", "__")):
                continue
            if name.startswith(REF_CHECK_PENDING):                # (the executed module defines them as stubs that throw: still pending)
                pending.append(name)
                continue
            if sym not in have and sym in other_units:
                reference.append(name)
                continue
            (resolved if sym in have else outside).append(name)
        drifted += [n for n in outside if n.startswith(REF_CHECK_NAMESPACES)]
        out[rel] = {"resolved": sorted(resolved), "outside": sorted(outside), "pending": sorted(pending), "reference": sorted(reference)}
    if drifted:
        raise RuntimeError("reference call sites name boundary functions the boundary does not define with that signature:\n" + "\n".join(drifted))
    # REPORT ONLY (VERDICT r04 missing 5 / item 9): the units above the model -- the Python binding, the batch generator, the model
    # context with its engine -- attempted against the same shim.  Nothing here fails the build: the report says how far each gets.
    report_objs, report_defined = {}, set()
    for rel in REF_REPORT_TUS:
        src = os.path.join(REFERENCE, rel)
        if not os.path.exists(src):
            continue
        obj = os.path.join(REFDIR, os.path.basename(src).rsplit(".", 1)[0] + ".report.o")
        r = subprocess.run(common + ["-c", src, "-o", obj], capture_output=True, text=True)
        if r.returncode != 0:
            errs = [ln for ln in r.stderr.splitlines() if " error" in ln or "fatal" in ln]
            out[rel] = {"report_only": True, "compiles": False, "errors": len(errs),
                        "first_errors": [e.replace(REFERENCE + "/", "").replace(PKG + "/", "") for e in errs[:6]]}
            continue
        report_objs[rel] = obj
        for line in subprocess.check_output(["nm", "--defined-only", obj], text=True).splitlines():
            report_defined.add(line.split()[-1])
    for rel, obj in report_objs.items():
        syms = [line.split()[-1] for line in subprocess.check_output(["nm", "-u", obj], text=True).splitlines()]
        os.remove(obj)
        names = subprocess.run(["c++filt"], input="\n".join(syms), text=True, capture_output=True).stdout.splitlines()
        res = [n for sy, n in zip(syms, names) if sy != n and sy in have]
        own = [n for sy, n in zip(syms, names) if sy != n and sy not in have and sy in report_defined]     # defined by another unit of the binding
        outside = [n for sy, n in zip(syms, names) if sy != n and sy not in have and sy not in report_defined
                   and not n.startswith(("std::", "operator ", "vtable for", "typeinfo for", "VTT for", "__", "pybind11::", "Py"))]
        out[rel] = {"report_only": True, "compiles": True, "resolved": sorted(res), "reference": sorted(own), "outside": sorted(outside)}
    with open(report, "w") as f:
        json.dump(out, f, indent=1)
    return report


def build(force=False, verbose=False):
    """every reference binary the tree can make (each step returns None without the reference tree and without a prebuilt file)"""
    build_refcompile(force, verbose)
    build_binding(force, verbose)
    return build_refcheck(force, verbose)


if __name__ == "__main__":
    zb.build(force="--force" in sys.argv, verbose=True)
