"""CPU: the one spelling of a launch entry point, dss2::entry (csrc/dss2_entry.hpp).

Completeness, from the sources: every function that include/dss2_hip.h declares with a ``void* stream`` parameter either goes through
dss2::entry (so it records into a launch plan), or refuses with DSS2_NOT_IN_PLAN, or is dss2_plan_run; nothing but the helper calls
plan_record; the spellings the helper replaced are gone.  The helper on its own: tests/entry_probe.cpp, a host program with stand-in
plan hooks, compiled with -fsanitize=address,undefined and run as a process."""
import glob
import os
import re
import shutil
import subprocess

import abi_probe
from conftest import PKG_NAME, ROOT

CSRC = os.path.join(ROOT, PKG_NAME, "csrc")


def _code(path):
    """A source file without its comments."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(path).read(), flags=re.S)


def _sources():
    return {os.path.basename(p): _code(p) for p in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.hpp")))}


def _declared():
    """{function: parameter text} of every prototype of the header."""
    return dict(re.findall(r"\b(dss2_\w+)\s*\(([^()]*)\)\s*;", abi_probe.header_text()))


def _definition(name, sources):
    """The body of ``extern "C" ... name(...) { ... }``, by brace matching."""
    found = []
    for text in sources.values():
        for m in re.finditer(r'extern\s+"C"\s+[\w\s\*]+?\b' + name + r"\s*\([^()]*\)\s*\{", text):
            depth, i = 1, m.end()
            while depth:
                depth += {"{": 1, "}": -1}.get(text[i], 0)
                i += 1
            found.append(text[m.end():i - 1])
    assert len(found) == 1, f"{name}: {len(found)} extern \"C\" definitions under csrc/"
    return found[0]


def test_every_entry_that_takes_a_stream_takes_part_in_plans():
    declared, sources = _declared(), _sources()
    streamed = [n for n, params in declared.items() if re.search(r"\bvoid\s*\*\s*stream\b", params)]
    print(f"[entry] {len(declared)} functions declared, {len(streamed)} take a stream")
    assert len(declared) == 110 and len(streamed) == 70
    how = {}
    for name in streamed:
        body = _definition(name, sources)
        how[name] = ("entry" if re.search(r"\bdss2::entry\s*\(", body) else "refuses" if re.search(r"\bDSS2_NOT_IN_PLAN\s*\(", body)
                     else "plan_run" if name == "dss2_plan_run" else None)
    assert not [n for n, h in how.items() if h is None], [n for n, h in how.items() if h is None]
    counts = {h: sum(1 for v in how.values() if v == h) for h in ("entry", "refuses", "plan_run")}
    print(f"[entry] {counts}")
    assert counts["plan_run"] == 1 and counts["entry"] + counts["refuses"] == 69
    # the refusal names the entry it sits in
    for name, h in how.items():
        if h == "refuses":
            assert re.search(r'DSS2_NOT_IN_PLAN\s*\(\s*"' + name + r'"\s*\)', _definition(name, sources)), name


def test_only_the_helper_records():
    sources = _sources()
    calls = {f: len(re.findall(r"\bplan_record\s*\(", re.sub(r"\bvoid\s+plan_record\s*\(", " ", text))) for f, text in sources.items()}
    assert {f: n for f, n in calls.items() if n} == {"dss2_entry.hpp": 1}
    for gone in ("DSS2_RECORD", "run_entry", "ws_entry", "plan_keep", "plan_ptr"):
        assert not [f for f, text in sources.items() if re.search(r"\b" + gone + r"\b", text)], gone
    # a launch body stands in front of its entry: no forward declaration of one
    assert not [m for text in sources.values() for m in re.findall(r"^static int \w+_launch\([^{;]*\);", text, flags=re.M)]


def test_the_helper_includes_no_hip():
    text = open(os.path.join(CSRC, "dss2_entry.hpp")).read()
    includes = re.findall(r"#\s*include\s*[<\"]([^>\"]+)[>\"]", text)
    assert includes and all("/" not in i and not i.startswith(("hip", "dss2")) for i in includes), includes


def test_entry_probe_under_sanitizers(tmp_path):
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
    cxx = next((p for p in map(shutil.which, ("c++", "g++", "clang++", rocm)) if p), None)
    assert cxx, "no C++ compiler for tests/entry_probe.cpp"
    exe = str(tmp_path / "entry_probe")
    # the sanitizer runtimes inside the program where the compiler has the flags for it (gcc; clang links them statically unasked):
    # a program then does not depend on the order in which the loader brings in shared libraries
    for static in (["-static-libasan", "-static-libubsan"], []):
        cc = subprocess.run([cxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                             *static, "-I", CSRC, os.path.join(ROOT, "tests", "entry_probe.cpp"), "-o", exe], capture_output=True, text=True)
        if cc.returncode == 0:
            break
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "entry_probe: ok", run.stdout + run.stderr
