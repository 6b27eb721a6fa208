"""CPU: csrc/knobs.h is the one place where libaocr.so reads its AOCR_* environment switches -- no other source file calls
getenv or names a switch in a string, DESIGN.md's switch table lists every declared switch once, the kernel tests' SWITCHES are all
declared, and each read kind means what the call sites it replaced meant (checked by a host-only program, tests/knobs_main.cc)."""
import ast
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "torch-attention-ocr_amd", "csrc")
KINDS = ("SET", "ON", "NOT0", "INT", "RAW")
# KNOB(NAME, KIND, DEFAULT, ...) / KNOB_CLAMP(NAME, KIND, DEFAULT, LO, HI, ...) / KNOB_ALSO(ACCESSOR, NAME, KIND, DEFAULT, ...)
_DECL = re.compile(r"^KNOB(_CLAMP|_ALSO)?\(\s*(\w+),\s*(\w+),\s*([^,]+?)\s*,", re.M)


def _read(path):
    with open(path, encoding="utf-8") as f:
        return f.read()


def _declared():
    """[(env name, kind, accessor)] in the header's order"""
    out = []
    for form, a, b, c in _DECL.findall(_read(os.path.join(CSRC, "knobs.h"))):
        out.append((b, c, a) if form == "_ALSO" else (a, b, a))
    return out


def test_header_declares_each_switch_once_with_a_known_kind():
    decl = _declared()
    assert len(decl) >= 90
    for name, kind, _ in decl:
        assert name.startswith("AOCR_") and kind in KINDS, (name, kind)
    accessors = [acc for _, _, acc in decl]
    assert len(set(accessors)) == len(accessors)
    primary = [name for name, _, acc in decl if acc == name]
    assert len(set(primary)) == len(primary), "a switch has two KNOB lines"
    assert {name for name, _, _ in decl} == set(primary), "KNOB_ALSO names a switch that has no KNOB line"
    # one line per declaration, and the header stays buildable by a host compiler alone
    text = _read(os.path.join(CSRC, "knobs.h"))
    assert re.findall(r"^\s*#\s*include\s*(\S+)", text, re.M) == ["<cstdlib>"]
    assert len([ln for ln in text.splitlines() if ln.startswith("KNOB")]) == len(decl)


def test_no_other_source_reads_the_environment():
    for fn in sorted(os.listdir(CSRC)):
        if fn == "knobs.h" or not os.path.isfile(os.path.join(CSRC, fn)):
            continue
        text = _read(os.path.join(CSRC, fn))
        assert "getenv(" not in text, f"csrc/{fn} calls getenv: add the switch to knobs.h"
        assert not re.search(r'"AOCR_\w*"', text), f"csrc/{fn} names a switch in a string literal: use its accessor"
    # inside the header: one getenv per kind and one in the clamped INT, each of a name the macro stringizes -- no table, loop or cache
    hdr = _read(os.path.join(CSRC, "knobs.h"))
    assert hdr.count("getenv(") == len(KINDS) + 1 and "static" not in hdr


def _design_rows():
    text = _read(os.path.join(ROOT, "DESIGN.md"))
    start = text.index("### Dispatch switches")
    end = text.index("\n## ", start)
    keys = []
    for ln in text[start:end].splitlines():
        if ln.startswith("| `AOCR_"):
            keys += re.findall(r"AOCR_[A-Z0-9_]+", ln.split("|")[1])
    return keys


def test_design_table_lists_every_switch_once():
    keys = _design_rows()
    dup = sorted({k for k in keys if keys.count(k) > 1})
    assert not dup, f"DESIGN.md lists these switches twice: {dup}"
    names = [name for name, _, acc in _declared() if acc == name]
    missing = [n for n in names if n not in keys]
    assert not missing, f"declared in knobs.h, not in DESIGN.md's switch table: {missing}"
    # in the header's order (the Python-side switches of the table come after them)
    assert [k for k in keys if k in names] == names


def test_kernel_test_switches_are_declared():
    tree = ast.parse(_read(os.path.join(ROOT, "tests", "kernel_harness.py")))
    value = next(n.value for n in tree.body if isinstance(n, ast.Assign) and any(getattr(t, "id", None) == "SWITCHES" for t in n.targets))
    switches = ast.literal_eval(value)
    assert len(switches) > 40
    names = {name for name, _, _ in _declared()}
    assert not [s for s in switches if s not in names]


def _host_cxx():
    for c in (shutil.which("c++"), shutil.which("g++"), shutil.which("clang++"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    cxx = _host_cxx()
    if cxx is None:
        pytest.skip("no host C++ compiler on this machine")
    exe = str(tmp_path_factory.mktemp("knobs") / "knobs_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-I" + CSRC, os.path.join(ROOT, "tests", "knobs_main.cc"), "-o", exe], check=True, capture_output=True)

    def run(**env):
        base = {k: v for k, v in os.environ.items() if not k.startswith("AOCR_")}
        base.update(env)
        out = subprocess.run([exe], env=base, check=True, capture_output=True, text=True).stdout
        return dict(ln.split("=", 1) for ln in out.splitlines())
    return run


# What each idiom of the call sites returned before the header existed, for the value None (unset), "", "0", "1", "2", "x":
#   SET   getenv(n) != nullptr                       ON    e && e[0] == '1'
#   NOT0  !(e && e[0] == '0')                        INT   e ? atoi(e) : default (AOCR_HALO4_STAGED: 7)
#   RAW   the pointer
VALUES = (None, "", "0", "1", "2", "x")
TRUTH = {
    "SET": ("0", "1", "1", "1", "1", "1"),
    "ON": ("0", "0", "0", "1", "0", "0"),
    "NOT0": ("1", "1", "0", "1", "1", "1"),
    "INT": ("7", "0", "0", "1", "2", "0"),
    "RAW": ("null", "[]", "[0]", "[1]", "[2]", "[x]"),
}
PROBED = {"SET": "AOCR_HALO8", "ON": "AOCR_NO_DMA", "NOT0": "AOCR_WGRAD_HALO_RAGGED", "INT": "AOCR_HALO4_STAGED", "RAW": "AOCR_ENC_BWD_RH"}


def test_probed_switches_have_the_kind_the_table_is_for():
    kinds = {name: kind for name, kind, acc in _declared() if acc == name}
    assert {k: kinds[n] for k, n in PROBED.items()} == {k: k for k in KINDS}


@pytest.mark.parametrize("i", range(len(VALUES)), ids=["unset", "empty", "0", "1", "2", "x"])
def test_kind_semantics(probe, i):
    v = VALUES[i]
    got = probe(**({} if v is None else {n: v for n in PROBED.values()}))
    assert {k: got[k] for k in KINDS} == {k: TRUTH[k][i] for k in KINDS}
    assert got["REREAD"] == "010"


def test_first_character_decides_on_and_not0(probe):
    got = probe(AOCR_NO_DMA="10", AOCR_WGRAD_HALO_RAGGED="01", AOCR_HALO4_STAGED="5x")
    assert (got["ON"], got["NOT0"], got["INT"]) == ("1", "0", "5")
    got = probe(AOCR_NO_DMA="01", AOCR_WGRAD_HALO_RAGGED="10", AOCR_HALO4_STAGED="-3")
    assert (got["ON"], got["NOT0"], got["INT"]) == ("0", "1", "-3")


@pytest.mark.parametrize("value,mink,cus", [(None, "192", "32"), ("", "32", "0"), ("0", "32", "0"), ("-5", "32", "0"), ("31", "32", "31"), ("33", "33", "33"),
                                            ("128", "128", "128"), ("129", "129", "128"), ("4096", "4096", "128"), ("x", "32", "0")])
def test_int_defaults_and_clamps(probe, value, mink, cus):
    # AOCR_F32W_MINK: mk ? max(32, atoi(mk)) : 192;  AOCR_COMM_RESERVE_CUS: n = e ? atoi(e) : 32, clamped to 0..128
    got = probe(**({} if value is None else {"AOCR_F32W_MINK": value, "AOCR_COMM_RESERVE_CUS": value}))
    assert (got["MINK"], got["CUS"]) == (mink, cus)


def test_one_name_read_two_ways_keeps_both(probe):
    # AOCR_DBG_STOP: cnn_backward / the g0 tap take atoi (0 = no stop); cnn_wgrad_on_side tested presence, so "0" kept the filter gradients off the side stream
    assert [(g["STOP"], g["STOP_SET"]) for g in (probe(), probe(AOCR_DBG_STOP="0"), probe(AOCR_DBG_STOP="2"))] == [("0", "0"), ("0", "1"), ("2", "1")]
