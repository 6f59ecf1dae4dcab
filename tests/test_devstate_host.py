"""Host checks of the per-device launch state (eemflow_amd/csrc/devstate.h): no GPU, no library load."""
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "eemflow_amd", "csrc")


def _sources():
    return {f: open(os.path.join(CSRC, f), encoding="utf-8").read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".h"))}


def _build_and_run(tmp_path, name):
    """tests/<name>.cpp as a stand-alone host program: no HIP, warnings are errors; it prints OK."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / name)
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", CSRC, os.path.join(REPO, "tests", name + ".cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


def test_devstate_decisions(tmp_path):
    """tests/devstate_check.cpp: when a kernel's dynamic-LDS limit is set again (a second device gets its own), and which scratch-arena
    slot serves a (device, stream) - with a counting fake for the HIP call, eight threads included."""
    _build_and_run(tmp_path, "devstate_check")


def test_stagerec_decisions(tmp_path):
    """tests/stagerec_check.cpp: what the stage recorder files and where, when a forward only measures and runs again, and when a
    stream call may continue the carried window - with a counting fake for the device copy."""
    _build_and_run(tmp_path, "stagerec_check")


def test_one_copy_of_each_piece_of_device_state():
    """The LDS limit, the CU count, the arena, the float buffer, the weight cursor and the packer are each written once."""
    src = _sources()
    where = lambda pat: sorted(f for f, text in src.items() if re.search(pat, text))
    assert where(r"hipFuncAttributeMaxDynamicSharedMemorySize") == ["devstate_hip.h"]
    assert where(r"multiProcessorCount") == ["devstate_hip.h"]
    assert where(r"static\s+(thread_local\s+)?(bool|int)\s+(raised|small_attr|attr)\b") == []
    for decl in (r"struct\s+Arena\b", r"struct\s+DevBuf\b", r"struct\s+Cursor\b", r"struct\s+Packer\b"):
        assert sum(len(re.findall(decl + r"\s*\{", text)) for text in src.values()) == 1, decl
    assert where(r"struct\s+(Buf|PBuf|Cur|Pk)\b") == []
    # the stage recorder, the stream carry, the create preamble, the 53-tap table and the contexts' buffer lifetime
    for decl in (r"struct\s+StageRec\b", r"struct\s+StageRecorder\b", r"struct\s+StreamCarry\b"):
        assert sum(len(re.findall(decl + r"\s*\{", text)) for text in src.values()) == 1, decl
    assert where(r"PlusStageRec") == []
    assert where(r"gcnArchName") == ["devstate_hip.h"]
    assert where(r"\bused\s*>") == ["stagerec.h"]                        # "this call only measured: run it again" is decided here ...
    assert where(r"rec_used") == []
    assert where(r"\boverflowed\(") == ["devstate_hip.h", "stagerec.h"]  # ... and asked through DevStageRecorder::rerun alone
    recorder = src["devstate_hip.h"].split("struct DevStageRecorder")[1].split("\n};")[0]
    assert "hipMemcpyAsync" in recorder and not re.search(r"<<<|LaunchKernel|_launch\(", recorder + src["stagerec.h"])   # it launches no kernel
    assert where(r"int\s+rec_stage\([^)]*\)\s*\{[^}]*hipMemcpy") == []    # no model copies a record itself
    assert where(r"->(carry_(on|h|w|wver|cin|padv)|stream_(pending|wver|h|w|pad))\b") == []   # StreamCarry's fields, kept by hand
    taps = r"\{\s*0,\s*2,\s*4,\s*6,\s*8,\s*10,\s*12,\s*14,\s*16,\s*18,\s*20,\s*21,"
    contexts = ("devstate.h", "devstate_hip.h", "ctx.h", "api.hip", "eraft_api.hip", "plus_api.hip", "workspace.hip", "schedule.hip")
    assert [f for f in contexts if re.search(taps, src[f])] == ["devstate.h"]
    for f in ("api.hip", "eraft_api.hip", "plus_api.hip"):
        assert not re.search(r"hipFree\([^;]*\.p\)", src[f]), f           # a DevBuf frees itself
        assert "ctx_open_device(" in src[f], f
