"""Code-object guard for bn_act_bwd_reduce_kernel (csrc/elementwise.hip), read from the built library on the CPU.

Its read-ahead loop issues the loads of the next row as inline asm and waits for them with a hand-counted `s_waitcnt vmcnt(NL)`: NL
loads per register set, in-order return, so vmcnt(NL) means "the older set has landed".  That count is right only while no other
vector-memory instruction sits inside the loop.  A compiler spill to scratch is one (scratch_store / scratch_load count in vmcnt), and
would make the wait release early: silently wrong, run-to-run different sums, no fault.  Every instantiation must therefore keep a zero
private segment and no VGPR spills."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "r-yolov4_amd", "csrc", "libryolo_hip.so")
BUNDLE_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _tool(name):
    d = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")          # the ROCm the library was built with (csrc/Makefile)
    if os.path.exists(os.path.join(d, name)):
        return os.path.join(d, name)
    path = shutil.which(name)
    assert path, f"{name} (ROCm LLVM tools) not found"
    return path


def _kernel_notes(tmp_path):
    """llvm-readelf --notes of every gfx950 code object in the library's .hip_fatbin section (one offload bundle per source file)."""
    assert os.path.exists(LIB), "libryolo_hip.so is not built (make -C r-yolov4_amd/csrc libryolo_hip.so)"
    fat = tmp_path / "fatbin"
    subprocess.check_call([_tool("llvm-objcopy"), f"--dump-section=.hip_fatbin={fat}", LIB, str(tmp_path / "lib_copy.so")])
    data = fat.read_bytes()
    starts = [m.start() for m in re.finditer(re.escape(BUNDLE_MAGIC), data)] + [len(data)]
    assert len(starts) > 1, "no offload bundle in .hip_fatbin"
    notes = []
    for i in range(len(starts) - 1):
        part, co = tmp_path / f"bundle{i}", tmp_path / f"bundle{i}.co"
        part.write_bytes(data[starts[i]:starts[i + 1]])
        subprocess.check_call([_tool("clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={part}", f"--output={co}"])
        notes.append(subprocess.run([_tool("llvm-readelf"), "--notes", str(co)], check=True, capture_output=True, text=True).stdout)
    return "\n".join(notes)


def _kernels(notes, needle):
    """{symbol: {field: value}} of the kernels whose symbol contains needle (fields of the AMDGPU metadata note)."""
    out = {}
    for block in re.split(r"\n\s*- \.agpr_count:", notes):
        m = re.search(r"\.name:\s+(\S+)", block)
        if m and needle in m.group(1):
            out[m.group(1)] = dict(re.findall(r"\.(private_segment_fixed_size|vgpr_spill_count|sgpr_spill_count|vgpr_count):\s+(\d+)", block))
    return out


def test_bn_act_bwd_reduce_kernel_has_no_scratch(tmp_path):
    ks = _kernels(_kernel_notes(tmp_path), "bn_act_bwd_reduce_kernel")
    assert len(ks) == 8, f"expected the 8 (activation x second branch) instantiations, found {sorted(ks)}"
    for name, f in ks.items():
        # the hand-counted vmcnt(NL) of the read-ahead loop holds only while no scratch access (spill) is a vector-memory op inside it
        assert f.get("private_segment_fixed_size") == "0", f"{name}: private segment {f.get('private_segment_fixed_size')} bytes"
        assert f.get("vgpr_spill_count") == "0", f"{name}: {f.get('vgpr_spill_count')} VGPR spills"
