"""The native library's environment switches: eemflow_amd/csrc/switches.def.h is the one inventory and switch.h the one reader.
Source text only (no library load), plus a stand-alone host program for the parse rules."""
import glob
import os
import re
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "eemflow_amd", "csrc")
NAME = r"EEM_[A-Z0-9_]+"


def _read(path):
    with open(path, errors="replace") as f:
        return f.read()


def _csrc_sources():
    return sorted(p for p in glob.glob(os.path.join(CSRC, "*")) if os.path.isfile(p))


def _rows():
    """{name: kind} of switches.def.h"""
    rows = dict(re.findall(r"^SW\((" + NAME + r"),\s*([A-Z0-9]+),", _read(os.path.join(CSRC, "switches.def.h")), re.M))
    assert len(rows) > 50, "switches.def.h did not parse"
    return rows


def _is_row(name, rows):
    return name in rows or any(kind == "FAMILY" and name.startswith(fam) for fam, kind in rows.items())


def test_only_switch_h_reads_the_environment():
    readers = [os.path.basename(p) for p in _csrc_sources() if "getenv" in _read(p)]
    assert readers == ["switch.h"], readers


def test_every_environment_name_in_csrc_is_a_row():
    """Quoted literals that start with EEM_ are environment names (error texts and kernel names start otherwise); the accessors take
    the enum, so outside the table such a literal is a read that went round it - or a message that names a switch, which must exist."""
    rows = _rows()
    unknown = {}
    for p in _csrc_sources():
        if p.endswith((".hip", ".h")):
            for name in re.findall(r'"(' + NAME + ")", _read(p)):
                if not _is_row(name.rstrip("_"), rows):
                    unknown.setdefault(os.path.basename(p), set()).add(name)
    assert not unknown, unknown
    # and every SW_EEM_* a site passes to an accessor is a row (the compiler says so too)
    for p in _csrc_sources():
        for name in re.findall(r"\bSW_(" + NAME + ")", _read(p)):
            assert name in rows, (os.path.basename(p), name)


def test_tests_and_tools_name_only_switches_that_exist():
    """A test or tool that sets a misspelt or removed switch compares a form with itself and passes.  Every EEM_* name under tests/,
    tools/ and in bench.py is a row of the table (or completes a family row), a variable a Python module of the package reads, a C macro
    of csrc/ or include/, or a variable of these files' own (one of them reads it through os.environ / os.getenv or a shell ${NAME...})."""
    rows = _rows()
    package_env = set()
    for p in glob.glob(os.path.join(REPO, "eemflow_amd", "*.py")):
        package_env |= set(re.findall(r"(?:environ(?:\.get|\.pop|\.setdefault)?\s*[\[(]|getenv\()\s*[\"'](" + NAME + ")", _read(p)))
    macros = set()
    for p in _csrc_sources() + glob.glob(os.path.join(REPO, "include", "*.h")):
        macros |= set(re.findall(r"#\s*(?:define|ifdef|ifndef|undef)\s+(" + NAME + ")", _read(p)))
        macros |= set(re.findall(r"defined\s*\(?\s*(" + NAME + ")", _read(p)))
    files = [os.path.join(REPO, "bench.py")]
    for sub in ("tests", "tools"):
        for root, _, names in os.walk(os.path.join(REPO, sub)):
            files += [os.path.join(root, n) for n in names if n.endswith((".py", ".sh", ".cpp", ".hip", ".h", ".md", ".txt"))]
    files = sorted(p for p in files if os.path.abspath(p) != os.path.abspath(__file__))
    texts = {p: _read(p) for p in files}
    own = set()                                                        # (one tool may export what another reads)
    for text in texts.values():
        own |= set(re.findall(r"(?:environ(?:\.get|\.pop|\.setdefault)?\s*[\[(]|getenv\()\s*[\"'](" + NAME + ")", text))
        own |= set(re.findall(r"\$\{(" + NAME + r")[:\-=?}]", text))
    unknown = {}
    for p, text in texts.items():
        for m in re.finditer(NAME, text):
            name, nxt = m.group(0), text[m.end():m.end() + 1]
            if name.endswith("_") and nxt in "*<{$%":                  # EEM_NO_*, EEM_ENC_PER_XCD_<tag>: a prefix of real names
                ok = any(r.startswith(name) for r in rows) or _is_row(name.rstrip("_"), rows)
            else:
                ok = _is_row(name, rows) or name in package_env or name in macros or name in own
            if not ok:
                unknown.setdefault(os.path.relpath(p, REPO), set()).add(name)
    assert not unknown, unknown


def test_no_dead_rows():
    rows = _rows()
    text = "".join(_read(p) for p in _csrc_sources() if p.endswith((".hip", ".h")) and not p.endswith(("switches.def.h", "switch.h")))
    dead = [name for name in rows if not re.search(r"\bSW_" + name + r"\b", text)]
    assert not dead, dead


def test_parse_rules(tmp_path):
    """tests/switch_parse_check.cpp: unset / "0" / "1" / "2" / "" for one switch of every parse kind, the families, and read-now
    against read-once accessors."""
    cxx = next((c for c in (os.environ.get("CXX"), "c++", "g++", "clang++", "/opt/rocm/lib/llvm/bin/clang++") if c and shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "switch_parse_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(REPO, "tests", "switch_parse_check.cpp"), "-o", exe],
                   check=True, capture_output=True, text=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("EEM_")}
    r = subprocess.run([exe], env=env, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "OK", r.stdout + r.stderr
