"""Builds libpn2_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
from __future__ import annotations

import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
INCLUDE = os.path.join(os.path.dirname(_HERE), "include")
LIB_PATH = os.path.join(_HERE, "libpn2_hip.so")
OBJ_DIR = os.path.join(CSRC, "build")

HIPCC_FLAGS = [
    "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
    # the only fused multiply-adds are the explicit __builtin_fmaf calls (index parity)
    "-ffp-contract=off",
    # IEEE-correct fp32 '/' and sqrtf (the hipcc default, stated because sdf.hip's bit parity depends on it)
    "-fhip-fp32-correctly-rounded-divide-sqrt",
    "-Wall", "-Wno-unused-function",
]


# Per-file additions.  sa_fused.hip: its only NaN-sensitive operations are ReLU / max-pool maxima, and in IEEE mode hipcc
# canonicalises every v_max operand first (v_max x, x, x): ~130 extra VALU instructions per tile in a kernel whose every
# non-MFMA instruction costs an issue slot of the matrix pipe's bubbles.  Arithmetic results are unchanged for non-NaN inputs.
PER_FILE_FLAGS = {"sa_fused.hip": ["-fno-honor-nans", "-mno-amdgpu-ieee"]}


_REMARK_CONTEXT = re.compile(r"^\s*(\d+ \||\|)")   # the source-line echo under a remark


def scratch_kernels(remarks: str) -> dict:
    """{mangled kernel name: scratch bytes per lane} for the kernels of a -Rpass-analysis=kernel-resource-usage compile
    whose ScratchSize is not zero."""
    bad, name = {}, None
    for line in remarks.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            continue
        m = re.search(r"remark:\s+ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name is not None and int(m.group(1)) != 0:
            bad[name] = int(m.group(1))
    return bad


def _hipcc() -> str:
    exe = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(exe):
        raise RuntimeError("hipcc not found: cannot build libpn2_hip.so")
    return exe


def sources() -> list[str]:
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".hip"))


def _deps_mtime() -> float:
    deps = sources() + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    deps += [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE) if f.endswith(".h")]
    return max(os.path.getmtime(p) for p in deps)


def build_variant(name: str, extra_flags, verbose: bool = False) -> str:
    """A tuning / profiling variant of the library: every source compiled with `extra_flags` on top of the product flags into
    its own object directory, linked as libpn2_hip.<name>.so next to the product library (never loaded unless PN2_LIB_PATH
    points at it: scripts/probes)."""
    return build(force=False, verbose=verbose, _variant=(name, list(extra_flags)))


def build(force: bool = False, verbose: bool = False, _variant=None) -> str:
    """Compile every .hip under csrc/ and link libpn2_hip.so.  Returns its path."""
    LIB_PATH, OBJ_DIR, vflags = globals()["LIB_PATH"], globals()["OBJ_DIR"], []
    if _variant is not None:
        LIB_PATH = os.path.join(_HERE, "libpn2_hip.%s.so" % _variant[0])
        OBJ_DIR = os.path.join(CSRC, "build", "variant_" + _variant[0])
        vflags = _variant[1]
    if not force and os.path.exists(LIB_PATH) and os.path.getmtime(LIB_PATH) >= _deps_mtime():
        return LIB_PATH
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    newest_hdr = max(
        [os.path.getmtime(os.path.join(CSRC, f)) for f in os.listdir(CSRC) if f.endswith(".h")]
        + [os.path.getmtime(os.path.join(INCLUDE, f)) for f in os.listdir(INCLUDE) if f.endswith(".h")]
    )

    def compile_one(src: str) -> str:
        obj = os.path.join(OBJ_DIR, os.path.basename(src)[:-4] + ".o")
        if (not force and os.path.exists(obj)
                and os.path.getmtime(obj) >= max(os.path.getmtime(src), newest_hdr)):
            return obj
        cmd = [hipcc, *HIPCC_FLAGS, *PER_FILE_FLAGS.get(os.path.basename(src), []),
               *os.environ.get("PN2_EXTRA_HIPCC_FLAGS", "").split(), *vflags, "-Rpass-analysis=kernel-resource-usage",
               "-c", src, "-o", obj]  # env: tuning sweeps
        if verbose:
            print(" ".join(cmd))
        p = subprocess.run(cmd, capture_output=True, text=True)
        diag = "\n".join(ln for ln in p.stderr.splitlines() if "-Rpass-analysis=kernel-resource-usage" not in ln
                         and not _REMARK_CONTEXT.match(ln))
        if diag.strip():
            print(diag, file=sys.stderr)
        if p.returncode:
            raise subprocess.CalledProcessError(p.returncode, cmd)
        # No kernel may use scratch (private) memory: a register array that hipcc leaves there costs 5-10x on a hot loop
        #  and is invisible in the source.  STRICT by default since round 6 (as a warning, a several-times
        # slower kernel shipped unnoticed from any build that did not go through __graft_entry__ or the tests): the build fails
        # and names the kernels.  Register allocation belongs to the toolchain, so the opt-out is explicit -- PN2_STRICT_SCRATCH=0
        # builds anyway and warns (a user's hipcc of another minor version that spills one register still gets a library).
        bad = scratch_kernels(p.stderr)
        if bad and os.environ.get("PN2_ALLOW_SCRATCH", "0") != "1":
            msg = "%s: kernels with scratch memory (bytes/lane): %s" % (os.path.basename(src), bad)
            if os.environ.get("PN2_STRICT_SCRATCH", "1") != "0":
                if os.path.exists(obj):
                    os.remove(obj)
                raise RuntimeError(msg + " -- the sources are held to zero scratch on ROCm 7.2's hipcc; PN2_STRICT_SCRATCH=0 builds "
                                   "anyway (expect these kernels to run several times slower)")
            print("hotrack_amd build WARNING: " + msg + " -- expect these kernels to run several times slower than on the "
                  "toolchain the sources were tuned with (ROCm 7.2 hipcc)", file=sys.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as ex:
        objs = list(ex.map(compile_one, sources()))
    tmp = LIB_PATH + ".tmp"
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", *objs, "-o", tmp])
    os.replace(tmp, LIB_PATH)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force=True, verbose=True))
