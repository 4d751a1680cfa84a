"""Build librerank_mi355.so in-tree with hipcc for gfx950 (no torch involved).

`python reranking-multimodal-retrievers_amd/build.py [--force]` or `build_library()` from Python.
The .so is git-ignored but travels to the GPU box with the gpurun snapshot.
"""
from __future__ import annotations

import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "librerank_mi355.so")
SOURCES = ["rr_api.hip", "bank_api.hip", "gemm_bf16.hip", "gemm_fp8.hip", "attention_bf16.hip", "elementwise.hip", "head.hip", "pair_assembly.hip", "li_scores.hip", "passage_bank.hip", "bank_search.hip", "bank_search_f16.hip", "bank_search_f16_plaid.hip", "bank_search_plaid.hip", "bank_compress.hip", "plaid_train.hip", "bank_ivf.hip", "bank_export.hip", "bank_merge.hip", "bank_move.hip",
           "pair_tokenizer.cpp"]
HEADERS = [os.path.join(CSRC, "rr_common.h"), os.path.join(os.path.dirname(HERE), "include", "rerank_mi355.h"),
           os.path.join(os.path.dirname(HERE), "include", "rerank_mi355_diag.h"),
           os.path.join(CSRC, "unicode_tables.h"), os.path.join(CSRC, "plaid_decode.h"), os.path.join(CSRC, "li_sources.h"),
           os.path.join(CSRC, "rank_order.h"), os.path.join(CSRC, "plaid_assign.h"), os.path.join(CSRC, "ivf_check.h"),
           os.path.join(CSRC, "rr_api_internal.h")]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -fno-slp-vectorize: no compiler-formed v_pk_*_f32.  Root cause of the corruption it was added for (round 2, ISA and
# measurements in profiles/r02_slp_hazard_isa.txt, tools/slp_hazard_probe.py): with SLP on, the LayerNorm-residual
# epilogue of the 128x128 GEMM compiles to `s_waitcnt vmcnt(2)` DIRECTLY followed by `v_pk_add_f32` on the registers the
# load just returned, and lanes 48-63 of the LOW register of the pair are intermittently read stale (16 rows x 1 column
# of a few tiles per launch).  One instruction between the wait and the first packed consumer cures it: the site
# (gemm_bf16.hip ln_apply) now carries an explicit `s_nop 1` behind the loads, so it is safe even with SLP on (verified:
# 0 wrong elements in 4 launches against 16-48 in each of 4).  The flag stays as the second line of defence: other
# epilogues add freshly loaded fp32 rows too, and hipcc's hazard recogniser does not know this pair.  Cost 0.7 % of the
# bench step.  Hand-written 2-wide vector code (the 32-row attention form's row sum) only touches VALU-produced values.
FLAGS = ["--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17", "-Wall", "-Wno-unused-function", "-fno-slp-vectorize",
         *os.environ.get("RR_HIPCC_EXTRA", "").split()]          # RR_HIPCC_EXTRA: A/B experiments only
# per-file extras: the attention softmax has no NaNs by construction; without IEEE-mode canonicalisation its 32-way row
# max is 16 v_max3_f32 instead of 54 instructions
EXTRA = {"attention_bf16.hip": ["-fno-honor-nans", "-mno-amdgpu-ieee"]}


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


OBJDUMP = os.path.join(os.path.dirname(os.path.dirname(HIPCC)), "lib", "llvm", "bin", "llvm-objdump")
# objects whose device code must hold NO packed-f32 arithmetic (see the -fno-slp-vectorize note above): every epilogue that adds
# freshly loaded fp32 / 16-bit rows lives in these.  attention_bf16 is exempt: its hand-written v_pk_add_f32 row sums only
# touch VALU-produced values (checked in the disassembly: the ones behind a vmcnt wait add the constant 0 to a row sum).
NO_PACKED_F32 = ["gemm_bf16.o", "gemm_fp8.o", "elementwise.o", "pair_assembly.o", "li_scores.o", "passage_bank.o", "bank_search.o", "bank_search_f16.o", "bank_search_f16_plaid.o", "bank_search_plaid.o", "bank_compress.o", "plaid_train.o", "bank_ivf.o", "bank_export.o", "bank_merge.o", "bank_move.o"]


def check_no_packed_f32(obj: str) -> None:
    """Fail the build if hipcc formed v_pk_{add,mul,fma}_f32 in `obj` (gfx950 hazard: a packed-f32 op directly behind the
    s_waitcnt vmcnt that released its source reads stale lanes 48-63; DESIGN.md "Numerics").  Guards against a build that
    lost -fno-slp-vectorize (RR_HIPCC_EXTRA experiments, a build not going through this script)."""
    import re
    import shutil
    import tempfile
    if not os.path.exists(OBJDUMP):
        raise RuntimeError(f"{OBJDUMP} not found: cannot verify the packed-f32 rule for {obj}")
    d = tempfile.mkdtemp(prefix="rr_isa_")
    try:
        local = os.path.join(d, os.path.basename(obj))
        shutil.copy(obj, local)
        subprocess.run([OBJDUMP, "--offloading", local], cwd=d, capture_output=True, text=True, check=True)
        dev = [f for f in os.listdir(d) if "gfx950" in f]
        if len(dev) != 1:
            raise RuntimeError(f"no gfx950 code object in {obj}")
        dis = subprocess.run([OBJDUMP, "-d", os.path.join(d, dev[0])], capture_output=True, text=True, check=True).stdout
        # Hand-written packed-f32 arithmetic exists in ONE place, the GELU Horner chain (rr_common.h gelu_erf_fast2: v_pk_fma_f32
        # only, every operand VALU-produced).  The rule the build enforces: no v_pk_add / v_pk_mul_f32 at all, and no v_pk_fma_f32
        # DIRECTLY behind an s_waitcnt (the measured failure is exactly that pair; one instruction in between cured it,
        # profiles/r02_slp_hazard_isa.txt).  A build that lost -fno-slp-vectorize violates both at once.  (Round 3 tried the
        # LayerNorm apply of the split residual body as packed operations: this check found `s_waitcnt vmcnt(1)` directly in
        # front of a packed subtract on freshly loaded fp32 residual rows; restricted to the VALU-fed form it was bit-identical and
        # bought 0.1 % — not kept.)
        bad = re.findall(r"v_pk_(?:add|mul)_f32[^\n]*", dis)
        ins = [l.split("//")[0].strip() for l in dis.splitlines() if l.startswith("\t")]
        for i, l in enumerate(ins):
            if i and l.startswith("v_pk_fma_f32") and ins[i - 1].startswith("s_waitcnt"):
                bad.append(l + "   (behind " + ins[i - 1] + ")")
        if bad:
            raise RuntimeError(f"{os.path.basename(obj)}: {len(bad)} packed-f32 instructions in the device code (first: {bad[0].strip()}); "
                               "build with -fno-slp-vectorize (reranking-multimodal-retrievers_amd/build.py FLAGS)")
    finally:
        shutil.rmtree(d, ignore_errors=True)


LAST_BUILD: dict = {}      # what the last build_library call did (also written to build/build_record.json)


def build_library(force: bool = False, verbose: bool = False) -> str:
    import json
    import time
    lib_existed = os.path.exists(LIB)
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    jobs = []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(objdir, os.path.splitext(s)[0] + ".o")
        if force or _stale(obj, [src] + HEADERS):
            if s.endswith(".cpp"):       # host-only C++ (no device code)
                jobs.append([HIPCC, "-O2", "-fPIC", "-std=c++17", "-Wall", "-pthread", "-c", src, "-o", obj])
            else:
                jobs.append([HIPCC, *FLAGS, *EXTRA.get(s, []), "-c", src, "-o", obj])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
        return r.stderr

    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(objdir, os.path.splitext(s)[0] + ".o") for s in SOURCES]
    if force or jobs or _stale(LIB, objs):
        # the ISA rule is checked on EVERY link, not only on the objects just compiled: an object that failed the check once
        # is removed, so that it can never be picked up as "up to date" by the next call (that happened: round 3)
        for o in NO_PACKED_F32:
            obj = os.path.join(objdir, o)
            try:
                check_no_packed_f32(obj)
            except RuntimeError:
                os.remove(obj)
                raise
        run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-pthread", "-o", LIB, *objs])
        linked = True
    else:
        linked = False
    LAST_BUILD.clear()
    LAST_BUILD.update(compiled=[os.path.basename(j[-3]) for j in jobs], linked=linked, reused_prebuilt_library=lib_existed and not linked,
                      forced=bool(force), when=time.strftime("%Y-%m-%dT%H:%M:%S"))
    try:
        with open(os.path.join(objdir, "build_record.json"), "w") as f:
            json.dump(LAST_BUILD, f, indent=1)
    except OSError:
        pass
    return LIB


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
