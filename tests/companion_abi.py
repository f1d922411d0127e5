"""What the CPU tests of the companion libraries (test_select_cpu, test_f64_cpu, test_query_cpu, test_foldin_cpu) share:
a library's names as its header declares them and as the .so exports them, the main library's for comparison, and a C99
program compiled against the header and run.  ``mod`` is the binding module (``simrank_amd._query`` ...)."""
import os
import re
import subprocess

from simrank_amd import _lib


def stem(mod) -> str:
    return re.fullmatch(r"libsimrank_(\w+)\.so", os.path.basename(mod.LIB_PATH)).group(1)


def header(mod) -> str:
    return open(mod.HEADER_PATH).read()


def declared(mod):
    """Sorted names the header declares with the library's API macro."""
    s = stem(mod)
    return sorted(set(re.findall(r"^SIMRANK_%s_API [\w \*]+?\b(simrank_%s_\w+)\(" % (s.upper(), s), header(mod), flags=re.M)))


def exported(lib_path):
    """Sorted names of every function the .so defines for others (``nm -D``): nothing but the API may be there."""
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    return sorted(set(re.findall(r" T (\w+)", out)))


def loaded_version(mod) -> int:
    """The version the loaded library reports, after checking that header, binding and exports name the same entries
    and that the header's version macro is the binding's."""
    assert declared(mod) == sorted(mod.PROTOTYPES)
    assert exported(mod.LIB_PATH) == declared(mod)
    assert re.search(r"#define SIMRANK_%s_VERSION %d\b" % (stem(mod).upper(), mod.VERSION), header(mod))
    return getattr(mod.load(), "simrank_%s_version" % stem(mod))()


def assert_header_stands_alone(mod):
    """Plain C with the two standard headers and nothing of the project's other headers."""
    text = header(mod)
    assert not re.findall(r'#include\s+"', text)
    assert set(re.findall(r"#include\s+<(\S+)>", text)) == {"stddef.h", "stdint.h"}


def assert_prototypes_match_the_header_argument_counts(mod):
    api = "SIMRANK_%s_API" % stem(mod).upper()
    for name, argtypes in mod.PROTOTYPES.items():
        m = re.search(r"^%s [\w \*]+?\b%s\(([^;]*?)\);" % (api, name), header(mod), flags=re.S | re.M)
        assert m, name
        args = m.group(1).strip()
        n = 0 if args == "void" else len(args.split(","))
        assert n == len(argtypes), (name, args)


def assert_links_nothing_of_the_main_library(mod):
    out = subprocess.run(["readelf", "-d", mod.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "NEEDED" in out and "libsimrank" not in out
    assert '#include "simrank_hip.h"' not in header(mod)


def main_library(mod):
    """(version the main library reports, names its header declares, names it exports), after checking that none of them
    is one of ``mod``'s library."""
    text = open(_lib.HEADER_PATH).read()
    names = set(re.findall(r"^SIMRANK_API [\w \*]+?\b(simrank_\w+)\(", text, flags=re.M))
    exports = set(exported(_lib.LIB_PATH))
    assert not [s for s in names | exports if s.startswith("simrank_" + stem(mod))]
    return _lib.load().simrank_abi_version(), names, exports


def run_c99(mod, tmp_path, source: str) -> str:
    """``source`` as a C99 program with every warning an error, linked to the library and run: its standard output."""
    s = stem(mod)
    src, exe = tmp_path / f"use_{s}.c", tmp_path / f"use_{s}"
    src.write_text(source)
    libdir = os.path.dirname(mod.LIB_PATH)
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", f"-I{os.path.dirname(mod.HEADER_PATH)}",
                         str(src), "-o", str(exe), f"-L{libdir}", f"-lsimrank_{s}", f"-Wl,-rpath,{libdir}"],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    return run.stdout


def layout_codes(mod) -> dict:
    """NAME -> value of the ``SIMRANK_<LIB>_<NAME> = value`` layout enumerators of the header."""
    found = re.findall(r"\bSIMRANK_%s_((?:PANEL|ROWMAJOR)_F\d+) = (\d+)" % stem(mod).upper(), header(mod))
    return {name: int(value) for name, value in found}
