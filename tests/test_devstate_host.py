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


def test_devstate_decisions(tmp_path):
    """tests/devstate_check.cpp: when a kernel's dynamic-LDS limit is set again (a second device gets its own), and which scratch-arena
    slot serves a (device, stream) - with a counting fake for the HIP call, eight threads included."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "devstate_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", CSRC, os.path.join(REPO, "tests", "devstate_check.cpp"),
                    "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr


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
