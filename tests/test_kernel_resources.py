"""What the compiler gave the kernels of the bench frame, read from the built library (no GPU): the gfx950 code object is taken out of libloupiote_hip.so with the ROCm
LLVM tools (llvm-objcopy, clang-offload-bundler) and its `amdhsa.kernels` metadata is read from llvm-readelf --notes.  Resource metadata only — no instruction is looked at.

k_shade re-reads its cold arguments from the argument segment so that the per-hit loop moves no scalar through VGPR lanes (kernels.h ShadeKernargs);
k_trace has done so since round 6 (TraceKernargs).  A change that brings the spills back fails here, before any GPU run.

k_trace_packet<false> is NOT held to zero SGPR spills, on purpose.  The same treatment took its 17 spills to 0 (78 SGPRs, 64 VGPRs as before), but its spilled scalars are
written and read once per PACKET, outside the node loop, and on the MI355X the kernel was no faster for it: 550.8 / 551.5 us a launch against 553.6 / 551.1 for the
parent, SQ_INSTS_VALU 290.47 M against 290.23 M a launch (profiles/r09_kernarg_ab.txt).  A restructure that only moves instructions is not kept, so the kernel is the
parent's and still reports 17; the test below only records that it keeps its 8 waves per SIMD and no scratch."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "loupiote_amd", "libloupiote_hip.so")
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"
TOOLS = ("llvm-objcopy", "clang-offload-bundler", "llvm-readelf")
FIELDS = ("name", "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "agpr_count", "private_segment_fixed_size")

# the instantiations bench.py's frame launches (mangled-name prefixes: the argument types follow)
K_SHADE = "_ZN4lptd7k_shadeILj0EE"                                # k_shade<0u>: no feature bit (kernel_forms.h)
K_PACKET = "_ZN4lptd14k_trace_packetILb0EE"                       # k_trace_packet<false>
K_TRACE = "_ZN4lptd7k_traceILb0ELb1ELb0ELb0EE"                    # k_trace<false, true, false, false>


def _tool_dir():
    roots = [os.environ.get(k) for k in ("ROCM_PATH", "HIP_PATH")]
    hipcc = shutil.which("hipcc")
    if hipcc:
        roots.append(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))))
    roots.append("/opt/rocm")
    for r in filter(None, roots):
        for sub in ("lib/llvm/bin", "llvm/bin"):
            d = os.path.join(r, sub)
            if all(os.path.exists(os.path.join(d, t)) for t in TOOLS):
                return d
    if all(shutil.which(t) for t in TOOLS):
        return os.path.dirname(shutil.which(TOOLS[0]))
    return None


@pytest.fixture(scope="module")
def kernels(tmp_path_factory):
    """mangled name -> {field: int} for every kernel of the library's gfx950 code object"""
    d = _tool_dir()
    if d is None:
        pytest.skip("the ROCm LLVM tools (%s) are not on this machine" % ", ".join(TOOLS))
    assert os.path.exists(LIB), "the library is not built (tests/conftest.py builds it)"
    tmp = tmp_path_factory.mktemp("code_object")
    fat, co = str(tmp / "lib.hip_fatbin"), str(tmp / "gfx950.co")
    subprocess.run([os.path.join(d, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fat, LIB, str(tmp / "rest.so")], check=True)
    subprocess.run([os.path.join(d, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fat, "--output=" + co, "--targets=" + TARGET], check=True)
    notes = subprocess.run([os.path.join(d, "llvm-readelf"), "--notes", co], check=True, capture_output=True, text=True).stdout
    assert "amdhsa.kernels:" in notes
    out = {}
    for rec in re.split(r"(?m)^  - (?=\.)", notes.split("amdhsa.kernels:", 1)[1])[1:]:
        f = dict(re.findall(r"(?m)^    \.(%s):\s+(\S+)\s*$" % "|".join(FIELDS), rec))      # four spaces: the kernel's own keys, not its arguments'
        name = f.pop("name", None)
        if name is not None:
            out[name] = {k: int(v) for k, v in f.items()}
    assert len(out) > 100, len(out)
    return out


def one(kernels, prefix):
    hit = [k for k in kernels if k.startswith(prefix)]
    assert len(hit) == 1, (prefix, hit)
    print(hit[0], kernels[hit[0]])
    return kernels[hit[0]]


def test_k_shade_of_the_bench_frame_spills_nothing_and_keeps_four_waves(kernels):
    k = one(kernels, K_SHADE)
    assert k["sgpr_spill_count"] == 0
    assert k["vgpr_count"] <= 128          # 4 waves per SIMD (kernel_forms.h shade_waves)
    assert k["private_segment_fixed_size"] == 0


def test_the_shading_kernels_exist_in_their_valid_forms_and_no_others(kernels):
    # kernel_forms.h: 96 of k_shade's 128 words are valid (ESAMP only with EMIS), k_path's 8 words with STATS off and on
    assert len([k for k in kernels if k.startswith("_ZN4lptd7k_shadeI")]) == 96
    assert len([k for k in kernels if k.startswith("_ZN4lptd6k_pathI")]) == 16


def test_k_trace_packet_of_the_bench_frame_keeps_eight_waves(kernels):
    k = one(kernels, K_PACKET)
    assert k["vgpr_count"] <= 64 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0


def test_k_trace_of_the_bench_frame_keeps_seven_waves_without_spills(kernels):
    k = one(kernels, K_TRACE)
    assert k["vgpr_count"] <= 72           # 7 waves per SIMD (512 / 7 = 73, in steps of 8)
    assert k["sgpr_spill_count"] == 0 and k["vgpr_spill_count"] == 0
