"""The one probe of the C ABI: include/dss2_hip.h as a C++ compiler lays it out, against the ctypes mirrors of _lib.py.

``mismatches(structs, signatures, constants)`` generates ONE C++17 file that includes the header, compiles it (nothing links against the
library: the functions enter through decltype alone), runs it and returns one line per disagreement:
  structs     {C struct tag: ctypes.Structure}      sizeof; offsetof, sizeof and kind of every field, by the field's name
  signatures  {function: (restype, argtypes)}       return kind, argument count, every argument's kind
  constants   {X: value}                            (long long) DSS2_X
A kind is ``i4`` / ``u8`` / ``f4`` (signed, unsigned, floating and the width; the header's enums count as signed), ``s:<struct tag>``,
``[n]<kind>`` for an array, ``v`` for void and ``p><kind>`` for a pointer, from decltype through <type_traits>.  ctypes' c_void_p and
c_char_p match any pointer; POINTER(S) must point to S's struct.  A name the header does not declare is reported and left out of the
generated file.  The caller passes the tables, so a test can also pass broken ones (tests/test_abi_cpu.py)."""
import ctypes as C
import functools
import keyword
import os
import re
import shutil
import subprocess
import tempfile

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "dss2_hip.h")
_PRELUDE = r"""
#include <cstddef>
#include <cstdio>
#include <type_traits>
#include "dss2_hip.h"
template <class T, class = void> struct K { static void p() { printf("?"); } };      // opaque types
template <> struct K<void> { static void p() { printf("v"); } };
template <class T> struct K<T, std::enable_if_t<std::is_arithmetic_v<T> || std::is_enum_v<T>>> {
  static void p() { printf("%c%zu", std::is_floating_point_v<T> ? 'f' : (std::is_enum_v<T> || std::is_signed_v<T>) ? 'i' : 'u', sizeof(T)); }
};
template <class T> struct K<T*> { static void p() { printf("p>"); K<std::remove_cv_t<T>>::p(); } };
template <class T, size_t N> struct K<T[N]> { static void p() { printf("[%zu]", N); K<std::remove_cv_t<T>>::p(); } };
template <class F> struct Sig;      // F = decltype(&function): unevaluated, so nothing has to link
template <class R, class... A> struct Sig<R (*)(A...)> {
  static void p(const char* name) { printf("F %s %zu ", name, sizeof...(A)); K<R>::p(); ((printf(" "), K<std::remove_cv_t<A>>::p()), ...); printf("\n"); }
};
#define STRUCT(T) template <> struct K<T> { static void p() { printf("s:" #T); } };
#define SIZE(T) printf("S " #T " %zu\n", sizeof(T));
#define FIELD(T, m) printf("M " #T "." #m " %zu %zu ", offsetof(T, m), sizeof(T::m)); K<std::remove_cv_t<decltype(T::m)>>::p(); printf("\n");
#define CONST(X) printf("C " #X " %lld\n", (long long)DSS2_##X);
"""


def header_text():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)


def header_struct_tags():
    """The names of ``typedef struct dss2_x {`` (the opaque dss2_plan has no body)."""
    return set(re.findall(r"typedef\s+struct\s+(dss2_\w+)\s*\{", header_text()))


def header_constants():
    """The DSS2_* macros (the include guard aside) and enumerators, without the prefix."""
    text = header_text()
    enums = " ".join(re.findall(r"\benum\s+\w+\s*\{(.*?)\}", text, flags=re.S))
    return set(re.findall(r"^\s*#\s*define\s+DSS2_(\w+)", text, flags=re.M)) - {"HIP_H"} | set(re.findall(r"\bDSS2_(\w+)", enums))


def c_name(field):
    """The C member a mirror's field stands for: a trailing underscore only where the C name is a Python keyword (lambda_)."""
    return field[:-1] if field.endswith("_") and keyword.iskeyword(field[:-1]) else field


def kind(t, tags):
    """The kind ctypes gives type t; tags: {ctypes.Structure: C struct tag}."""
    if t is None or t in (C.c_void_p, C.c_char_p):
        return "v" if t is None else "p"
    if issubclass(t, C.Structure):
        return "s:" + tags.get(t, "?" + t.__name__)
    if issubclass(t, (C.Array, C._Pointer)):
        return (f"[{t._length_}]" if issubclass(t, C.Array) else "p>") + kind(t._type_, tags)
    return ("f" if t._type_ in "fd" else "i" if t._type_.islower() else "u") + str(C.sizeof(t))


def same_kind(mirror, header):
    """A bare ``p`` on the mirror's side (c_void_p, c_char_p) is any pointer."""
    return mirror == header or (mirror.endswith("p") and header.startswith(mirror + ">"))


@functools.lru_cache(maxsize=None)
def _run(source):
    """(output, "") of the compiled source, or (None, the compiler's errors); the same text is compiled once per session."""
    rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")      # the one hipcc itself runs
    cxx = next((p for p in map(shutil.which, ("c++", "g++", "clang++", rocm)) if p), None)
    if cxx is None:
        raise RuntimeError("no C++ compiler (c++, g++, clang++, ROCm's clang++) to check the mirrors against include/dss2_hip.h")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "abi.cpp"), os.path.join(d, "abi")
        with open(src, "w") as fh:
            fh.write(source)
        cc = subprocess.run([cxx, "-std=c++17", "-I", os.path.dirname(HEADER), src, "-o", exe], capture_output=True, text=True)
        if cc.returncode != 0:
            return None, cc.stderr
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout, ""


def mismatches(structs, signatures, constants):
    """One line per disagreement between the header and the given tables; [] when they agree."""
    text, tags, bad = header_text(), {cls: tag for tag, cls in structs.items()}, []

    def declared(table, pattern, what):
        bad.extend(f"{what.format(n)}: not declared in include/dss2_hip.h" for n in table if not re.search(pattern.format(n), text))
        return {n: v for n, v in table.items() if re.search(pattern.format(n), text)}

    structs = declared(structs, r"\}}\s*{}\s*;", "struct {}")
    signatures = declared(signatures, r"\b{}\s*\(", "function {}")
    constants = declared(constants, r"\bDSS2_{}\b", "constant DSS2_{}")
    lines = [_PRELUDE] + [f"STRUCT({tag})" for tag in structs] + ["int main() {"]
    for tag, cls in structs.items():
        lines += [f"SIZE({tag})"] + [f"FIELD({tag}, {c_name(f)})" for f, _ in cls._fields_]
    lines += [f'Sig<decltype(&{name})>::p("{name}");' for name in signatures] + [f"CONST({name})" for name in constants] + ["return 0;", "}"]
    out, err = _run("\n".join(lines) + "\n")
    if out is None:
        return bad + ["the probe does not compile (a field or a name the header does not have?):\n" + err]
    got = {" ".join(ln.split()[:2]): ln.split()[2:] for ln in out.splitlines()}
    for tag, cls in structs.items():
        if int(got[f"S {tag}"][0]) != C.sizeof(cls):
            bad.append(f"struct {tag}: header sizeof {got[f'S {tag}'][0]}, mirror {cls.__name__} sizeof {C.sizeof(cls)}")
        for f, t in cls._fields_:
            (off, sz, k), d = got[f"M {tag}.{c_name(f)}"], getattr(cls, f)
            if (int(off), int(sz)) != (d.offset, d.size) or not same_kind(kind(t, tags), k):
                bad.append(f"struct {tag} field {c_name(f)}: header offset {off} size {sz} kind {k}, "
                           f"mirror {cls.__name__}.{f} offset {d.offset} size {d.size} kind {kind(t, tags)}")
    for name, (res, args) in signatures.items():
        n, *ks = got[f"F {name}"]
        if int(n) != len(args):
            bad.append(f"function {name}: header takes {n} arguments, mirror {len(args)}")
        bad += [f"function {name} {'return' if i == 0 else f'argument {i - 1}'}: header {k}, mirror {kind(a, tags)}"
                for i, (a, k) in enumerate(zip([res] + list(args), ks)) if not same_kind(kind(a, tags), k)]
    return bad + [f"constant {name}: header DSS2_{name} = {got[f'C {name}'][0]}, mirror {v}"
                  for name, v in constants.items() if int(got[f"C {name}"][0]) != v]
