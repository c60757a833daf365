"""In-tree build of the HIP library (hipcc, gfx950 only).  No JIT cache: the
resulting audiosignalprocess_amd/lib/libasp_amd.so travels with the tree."""
import glob
import os
import shutil
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIBDIR = os.path.join(PKG, "lib")
# ASP_AMD_LIB: load another build of the library (same-box A / B runs against an earlier build)
LIB = os.environ.get("ASP_AMD_LIB") or os.path.join(LIBDIR, "libasp_amd.so")
SOURCES = ["ns_kernels.hip", "ns_kernels1.hip", "ns_kernels2.hip", "ns_kernels_hb.hip", "ns_api.hip", "bt_kernels.hip", "bt_kernels8.hip", "bt_api.hip",
           "aec_kernels.hip", "aec_delay_kernels.hip", "aec_api.hip", "qmf_kernels.hip", "qmf_api.hip", "sinc_kernels.hip", "sinc_api.hip",
           "vad_kernels.hip", "vad_api.hip", "aecm_kernels.hip", "aecm_api.hip", "nsx_kernels.hip", "nsx_api.hip",
           "splrs_kernels.hip", "splrs_api.hip", "agc_kernels.hip", "agc_api.hip", "ts_kernels.hip", "ts_api.hip",
           "bf_kernels.hip", "bf_api.hip", "hpf_kernels.hip", "hpf_api.hip", "level_kernels.hip", "level_api.hip",
           "ab_kernels.hip", "ab_api.hip"]
C_SOURCES = ["wav_io.c"]  # host-only C (kept C, as in the reference)
# -ffp-contract=off: parity with the reference depends on unfused mul/add.
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-fPIC", "-std=c++17",
         "-Wall", "-Wno-unused-function"]


# per-file extras; ASP_HIPCC_EXTRA="file.hip:-flag -flag;other.hip:-flag" adds more (experiments)
# kernarg preload (gfx950): the dispatch arrives with its arguments in SGPRs instead of fetching them
# with dependent scalar loads before the first vector load can issue (-0.5 us per NS step, measured);
# the object carries a prologue for firmware without the feature
_PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=8"]
EXTRA = {"ns_kernels.hip": list(_PRELOAD),
         # the hand-off build's step loop: machine LICM hoists the fp64 constants of the whole frame step in front of it
         # and they spill (60 VGPRs); without it both hand-off instantiations hold 128 VGPRs, no spill, no scratch
         # (profiles/r05_ns_walk_resource_usage.txt)
         "ns_kernels1.hip": list(_PRELOAD) + ["-mllvm", "-disable-machine-licm"],
         "ns_kernels2.hip": list(_PRELOAD),
         # the echo canceller's block is long straight-line code at 4 waves per SIMD: the compiler's ILP-first
         # scheduling measured 92.7-93.8 us per step against 95.5 us in one session (max-ilp: 97-99 us)
         "aec_kernels.hip": ["-mllvm", "-amdgpu-sched-strategy=iterative-ilp"],
         # the echo canceller's per-lane code: unrolled, its 65-bin loops spill to scratch (564 B); rolled, none
         "aecm_kernels.hip": ["-fno-unroll-loops"]}
# second builds of a source under another object name: (source, object, extra flags)
VARIANTS = []
for _item in filter(None, os.environ.get("ASP_HIPCC_EXTRA", "").split(";")):
    _f, _, _fl = _item.partition(":")
    EXTRA.setdefault(_f.strip(), []).extend(_fl.split())


def hipcc():
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: the HIP library cannot be built")
    return exe


def _stale(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build_library(force=False, verbose=False):
    """Compile csrc/*.hip into lib/libasp_amd.so; returns its path."""
    os.makedirs(LIBDIR, exist_ok=True)
    srcs = [os.path.join(CSRC, s) for s in SOURCES]
    hdrs = sorted(glob.glob(os.path.join(CSRC, "*.h")) + glob.glob(os.path.join(ROOT, "include", "*.h")))
    objs = []
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    for s in srcs:
        o = os.path.join(LIBDIR, os.path.basename(s) + ".o")
        if force or _stale(o, [s] + hdrs):
            cmd = [hipcc()] + FLAGS + EXTRA.get(os.path.basename(s), []) + inc + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
        objs.append(o)
    for src_name, obj_name, flags in VARIANTS:
        s = os.path.join(CSRC, src_name)
        o = os.path.join(LIBDIR, obj_name)
        if force or _stale(o, [s] + hdrs):
            cmd = [hipcc()] + FLAGS + EXTRA.get(src_name, []) + flags + inc + ["-c", s, "-o", o]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
        objs.append(o)
    for s in C_SOURCES:
        src = os.path.join(CSRC, s)
        o = os.path.join(LIBDIR, s + ".o")
        if force or _stale(o, [src, os.path.join(ROOT, "include", "wav_io.h")]):
            cmd = ["gcc", "-O2", "-std=gnu99", "-fPIC", "-Wall"] + inc + ["-c", src, "-o", o]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
        objs.append(o)
    # the CPU builds of the AECM, NSX, resampler, gain-control, transient-suppressor, beamformer, high-pass filter / level
    # estimator and audio buffer cores, for the tests only (no CPU path in libasp_amd.so)
    for src_name, so_name in (("aecm_restate.cpp", "libaecm_restate.so"), ("nsx_restate.cpp", "libnsx_restate.so"),
                              ("splrs_restate.cpp", "libsplrs_restate.so"), ("agc_restate.cpp", "libagc_restate.so"),
                              ("ts_restate.cpp", "libts_restate.so"), ("bf_restate.cpp", "libbf_restate.so"),
                              ("hpf_restate.cpp", "libhpf_restate.so"), ("ab_restate.cpp", "libab_restate.so")):
        src = os.path.join(CSRC, src_name)
        so = os.path.join(LIBDIR, so_name)
        if force or _stale(so, [src] + hdrs):
            cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall"] + inc + [src, "-o", so]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
    if force or _stale(LIB, objs):
        cmd = [hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    return LIB


def build_drivers(verbose=False):
    """The C and C++ drivers (drivers/*.c, drivers/*.cpp) linked against the in-tree library."""
    out_dir = os.path.join(ROOT, "drivers", "bin")
    os.makedirs(out_dir, exist_ok=True)
    built = []
    # (name, header or None). The .c drivers link the C ABI; the .cpp ones are clients of the header-only classes
    # APM_NS (include/apm_ns.h) and webrtc::Resampler (include/webrtc_resampler.h). Callers index this list from both
    # ends (test_ns_module first, test_vad_module and apm_ns_raw last), so new drivers go in the middle.
    drivers = [("test_ns_module", None), ("ns_batch_wav", None), ("test_aec_module", None), ("bt_main", None),
               ("test_aecm_module", None), ("test_nsx_module", None), ("test_resampler_module", "webrtc_resampler.h"),
               ("test_vad_module", None), ("apm_ns_raw", "apm_ns.h")]
    for name, header in drivers:
        src = os.path.join(ROOT, "drivers", name + (".cpp" if header else ".c"))
        exe = os.path.join(out_dir, name)
        deps = [src, LIB] + ([os.path.join(ROOT, "include", header)] if header else [])
        if _stale(exe, deps):
            cc = ["g++", "-O2", "-std=c++11"] if header else ["gcc", "-O2", "-std=gnu99"]
            cmd = cc + ["-Wall", "-I" + os.path.join(ROOT, "include"), src,
                        "-L" + LIBDIR, "-lasp_amd", "-Wl,-rpath,$ORIGIN/../../audiosignalprocess_amd/lib",
                        "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe]
            if verbose:
                print(" ".join(cmd))
            subprocess.run(cmd, check=True)
        built.append(exe)
    return built


if __name__ == "__main__":
    print(build_library(verbose=True))
    print(build_drivers(verbose=True))
