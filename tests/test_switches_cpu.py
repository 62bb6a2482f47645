"""CPU-only: the table of OCRL_* environment switches (csrc/switches.h) and its readers, through a stand-alone host program built with
the Makefile's compiler; and the table against the sources and INTEGRATION.md.  EXPECT below is written out from the sites as they read
the environment before the table existed (name: default when unset, moment of reading) -- not generated from the header.  No device is
touched.  To run the program under the sanitizers, add "-fsanitize=address,undefined" to FLAGS."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ocrl_amd", "csrc")
FLAGS = ["-x", "c++", "-std=c++17", "-O1"]

EXPECT = {
    "OCRL_GEMM_TILE": (0, "PROCESS"), "OCRL_GEMM_SB": (0, "PROCESS"), "OCRL_CONV_LAT": (1, "PROCESS"), "OCRL_BC_WGRAD": (2, "PROCESS"),
    "OCRL_SA_GROUP": (1, "PROCESS"), "OCRL_SA_WGS": (0, "PROCESS"), "OCRL_SA_FWD": (2, "PROCESS"), "OCRL_SA_BWD": (2, "PROCESS"),
    "OCRL_CONV_X3": (0, "MODEL"), "OCRL_ENCODE_GRAPH": (0, "MODEL"), "OCRL_ATTN_DS_MB": (2048, "MODEL"), "OCRL_OVERLAP": (5, "MODEL"),
    "OCRL_DW_SIDE": (2, "MODEL"), "OCRL_TOKENS_LATE": (0, "MODEL"), "OCRL_SA_INPUT": (1, "MODEL"), "OCRL_XATTN": (1, "MODEL"),
    "OCRL_ATTN_BWD": (0, "CALL"), "OCRL_SA_NS": (0, "CALL"),
}

# `table`: name, default, moment of every row.  `read`: every row through the reader of its moment.  `twice <text> <tile text>`: every
# row read, the variable set to <text> (OCRL_GEMM_TILE: <tile text>), and read again -- plus OCRL_CONV_X3 through its second, per-process reader
PROGRAM = r"""
#include "switches.h"
#include <string.h>

template <sw::Switch S>
static long long rd() {
    if constexpr (sw::TABLE[S].when == sw::PROCESS) return sw::process<S>();
    else if constexpr (sw::TABLE[S].when == sw::MODEL) return sw::model<S>();
    else return sw::call<S>();
}
template <sw::Switch S>
static void twice(const char* text, const char* tile) {
    const long long a = rd<S>();
    setenv(sw::TABLE[S].name, S == sw::OCRL_GEMM_TILE ? tile : text, 1);
    printf("%s %lld %lld\n", sw::TABLE[S].name, a, rd<S>());
}
int main(int argc, char** argv) {
    static const char* const MOMENT[] = {"PROCESS", "MODEL", "CALL"};
    if (argc == 2 && !strcmp(argv[1], "table")) {
        for (const sw::Row& r : sw::TABLE) printf("%s %lld %s\n", r.name, r.def, MOMENT[r.when]);
    } else if (argc == 2 && !strcmp(argv[1], "read")) {
#define X(name, def, when, meaning) printf("%s %lld\n", #name, rd<sw::name>());
        OCRL_SWITCHES(X)
#undef X
    } else if (argc == 4 && !strcmp(argv[1], "twice")) {
        const long long x3 = sw::process<sw::OCRL_CONV_X3>();
#define X(name, def, when, meaning) twice<sw::name>(argv[2], argv[3]);
        OCRL_SWITCHES(X)
#undef X
        printf("OCRL_CONV_X3/process %lld %lld\n", x3, sw::process<sw::OCRL_CONV_X3>());
    } else return 2;
    return 0;
}
"""


def compiler():
    default = re.search(r"^HIPCC \?= (\S+)", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1)
    return os.environ.get("HIPCC", default)


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("switches")
    src, exe = d / "switches_prog.cpp", d / "switches_prog"
    src.write_text(PROGRAM)
    subprocess.run([compiler(), *FLAGS, "-I", CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)

    def run(*args, **env):
        clean = {k: v for k, v in os.environ.items() if not k.startswith("OCRL_")}
        out = subprocess.run([str(exe), *args], env={**clean, **env}, check=True, capture_output=True, text=True).stdout
        return {f[0]: tuple(f[1:]) for f in (line.split() for line in out.splitlines())}
    return run


def text_for(name, number):
    return f"{number}x64" if name == "OCRL_GEMM_TILE" else str(number)


def test_table_is_the_expected_one(prog):
    assert prog("table") == {n: (str(d), m) for n, (d, m) in EXPECT.items()}


def test_unset_gives_the_default(prog):
    assert prog("read") == {n: (str(d),) for n, (d, _) in EXPECT.items()}


def test_set_gives_the_value(prog):
    want = {n: ("7",) for n in EXPECT}
    want["OCRL_GEMM_TILE"] = ("7064",)
    want["OCRL_TOKENS_LATE"] = ("1",)           # its presence is the switch
    assert prog("read", **{n: text_for(n, 7) for n in EXPECT}) == want
    assert prog("read", OCRL_ATTN_DS_MB="8589934592")["OCRL_ATTN_DS_MB"] == ("8589934592",)       # the one 64-bit value
    assert prog("read", OCRL_TOKENS_LATE="0")["OCRL_TOKENS_LATE"] == ("1",)
    assert prog("read", OCRL_SA_NS="-3", OCRL_XATTN=" 12abc") == {**{n: (str(d),) for n, (d, _) in EXPECT.items()},
                                                                 "OCRL_SA_NS": ("-3",), "OCRL_XATTN": ("12",)}


def test_text_that_is_no_number_gives_zero(prog):
    want = {n: ("0",) for n in EXPECT}
    want["OCRL_TOKENS_LATE"] = ("1",)
    assert prog("read", **{n: "junk" for n in EXPECT}) == want


def test_gemm_tile_parse(prog):
    assert prog("read", OCRL_GEMM_TILE="128x64")["OCRL_GEMM_TILE"] == ("128064",)
    assert prog("read", OCRL_GEMM_TILE="junk")["OCRL_GEMM_TILE"] == ("0",)
    assert prog("read", OCRL_GEMM_TILE="128")["OCRL_GEMM_TILE"] == ("0",)


@pytest.mark.parametrize("start", ["unset", "set"])
def test_moment_of_reading(prog, start):
    """the variable changes between two reads: a PROCESS switch keeps what it read first, MODEL and CALL switches see the new text"""
    env = {n: text_for(n, 3) for n in EXPECT} if start == "set" else {}
    got = prog("twice", "4", "4x64", **env)
    for n, (d, moment) in EXPECT.items():
        first = ("3064" if n == "OCRL_GEMM_TILE" else "1" if n == "OCRL_TOKENS_LATE" else "3") if start == "set" else str(d)
        new = "4064" if n == "OCRL_GEMM_TILE" else "1" if n == "OCRL_TOKENS_LATE" else "4"
        assert got[n] == (first, first if moment == "PROCESS" else new), n
    x3 = "3" if start == "set" else "0"
    assert got["OCRL_CONV_X3/process"] == (x3, x3)        # conv_wgrad_launch's fallback: once per process


def sources():
    return {f: open(os.path.join(CSRC, f)).read() for f in sorted(os.listdir(CSRC)) if f.endswith((".hip", ".cpp", ".h"))}


def test_table_names_are_the_switch_names_in_the_sources():
    """every OCRL_* token of csrc/ is a row of the table, unless it is a macro: a constant of the C ABI (#define in include/ocrl_hip.h)
    or one of csrc/'s own (#define: OCRL_REQUIRE, OCRL_HIP, ...) -- an environment name is never #defined"""
    src = sources()
    macros = set(re.findall(r"#\s*define\s+(OCRL_[A-Z0-9_]+)", open(os.path.join(ROOT, "include", "ocrl_hip.h")).read()))
    macros |= {m for text in src.values() for m in re.findall(r"#\s*define\s+(OCRL_[A-Z0-9_]+)", text)}
    tokens = {t for text in src.values() for t in re.findall(r"OCRL_[A-Z0-9_]+", text)}
    assert tokens - macros == set(EXPECT)
    rows = re.findall(r"^\s*X\((OCRL_[A-Z0-9_]+),", src["switches.h"], re.M)
    assert sorted(rows) == sorted(EXPECT) and len(rows) == 18


def test_only_the_header_reads_the_environment():
    assert [f for f, text in sources().items() if "getenv(" in text] == ["switches.h"]


def test_integration_md_has_every_row():
    """| `OCRL_NAME` | default | moment | ... one row per switch, the same default and moment as the header"""
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    rows = {m.group(1): (int(m.group(2)), m.group(3)) for m in re.finditer(r"^\| `(OCRL_[A-Z0-9_]+)` \| (-?\d+) \| (\w+) \|", doc, re.M)}
    assert rows == EXPECT
