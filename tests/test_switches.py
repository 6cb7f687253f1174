"""The SX_* environment switches have one owner: stringsext_amd/csrc/sx_switches.hpp is the list, sx_switches.cpp the only reader,
and a context keeps the snapshot sx_create took (no GPU needed: the last test drives a host-only context)."""
import glob
import os
import random
import re

import refconfig as rc
import stringsext_amd as sx
from product_harness import oracle_runs_for_chunk
from test_wave_core import text_lines

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stringsext_amd", "csrc")

# names that look like switches and are read by Python, never by the library
PYTHON_ONLY = {"SX_LIB", "SX_WRITE_TABLE_REPORT", "SX_GATHER_SEG_BYTES"}
PYTHON_ONLY_PREFIXES = ("SX_FUZZ_",)


def table_names():
    """the table: one field per line, its comment begins with the switch's name"""
    text = open(os.path.join(CSRC, "sx_switches.hpp"), encoding="utf-8").read()
    names = re.findall(r";\s*// (SX_[A-Z0-9_]+)", text)
    assert len(names) == len(set(names)) >= 60, names
    return set(names)


def test_the_library_reads_the_environment_in_one_file_only():
    readers = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*"))
                     if os.path.isfile(p) and "getenv(" in open(p, encoding="utf-8", errors="replace").read())
    assert readers == ["sx_switches.cpp"]
    # ... and that file reads exactly the names of the table
    parsed = set(re.findall(r'"(SX_[A-Z0-9_]+)"', open(os.path.join(CSRC, "sx_switches.cpp"), encoding="utf-8").read()))
    assert parsed == table_names()


def names_set_as_environment(text):
    """SX_* string literals a Python or shell source sets as an environment variable: os.environ[...] = / .pop / .update(dict or keywords),
    monkeypatch.setenv / delenv, dict literals of switches ({"SX_X": "1"}), NAME=value in front of a shell command, export NAME=..."""
    found = set()
    found |= set(re.findall(r"""environ\[["'](SX_[A-Z0-9_]+)["']\]\s*=[^=]""", text))
    found |= set(re.findall(r"""(?:setenv|delenv|environ\.pop|environ\.setdefault)\(["'](SX_[A-Z0-9_]+)["']""", text))
    found |= set(re.findall(r"""["'](SX_[A-Z0-9_]+)["']\s*:\s*["']""", text))          # {"SX_X": "value"}: the switch sets of tests and fuzz
    found |= set(re.findall(r"""\bdict\([^)]*?\b(SX_[A-Z0-9_]+)=""", text))
    found |= set(re.findall(r"""(?:^|[\s;(])(?:export\s+)?(SX_[A-Z0-9_]+)=""", text, flags=re.M))   # shell, and keyword arguments of environ.update()
    return found


def test_every_switch_a_test_or_tool_sets_is_in_the_table():
    known = table_names()
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.sh"))
    assert len(files) > 30
    unknown = {}
    n_set = 0
    for path in files:
        if os.path.basename(path) == "test_switches.py":
            continue
        for name in names_set_as_environment(open(path, encoding="utf-8", errors="replace").read()):
            n_set += 1
            if name in known or name in PYTHON_ONLY or name.startswith(PYTHON_ONLY_PREFIXES):
                continue
            unknown.setdefault(name, []).append(os.path.relpath(path, ROOT))
    assert n_set > 60           # (the patterns above do find the switch sets)
    assert not unknown, f"set as environment variables but not in sx_switches.hpp (a misspelt switch does nothing, silently): {unknown}"


def test_the_detector_sees_every_way_of_setting_a_switch():
    src = '''
os.environ["SX_AA"] = "1"
monkeypatch.setenv("SX_BB", "0"); monkeypatch.delenv("SX_CC", raising=False); os.environ.pop("SX_DD", None)
SETS = [{}, {"SX_EE": "2", "SX_FF": "1"}]
env = dict(os.environ, SX_GG="1")
if os.environ["SX_NOT_SET"] == "1": pass
SX_HH=1 SX_II=0 python bench.py
export SX_JJ=3
'''
    assert names_set_as_environment(src) == {"SX_AA", "SX_BB", "SX_CC", "SX_DD", "SX_EE", "SX_FF", "SX_GG", "SX_HH", "SX_II", "SX_JJ"}


def n_segments_of_a_host_merge(sc, ms, data):
    res = sc.replay_runs(data, oracle_runs_for_chunk(ms, data, 0), file_id=1, is_last=True)
    try:
        assert sum(len(arena) for _, _, arena in res.segments()) > 100_000   # (strings of both Missions: several segments of 20 000 bytes' worth)
        return len(res.segments())
    finally:
        res.free()


def test_a_context_keeps_the_switches_it_was_created_under(monkeypatch):
    """SX_HOST_MERGE_SEG_BYTES cuts the interleaved result of a host-only context with two Missions into segments: the context created
    under it goes on cutting after the variable is gone, and the one created without it does not begin to when it appears"""
    monkeypatch.delenv("SX_HOST_MERGE_SEG_BYTES", raising=False)
    ms = rc.missions(encodings=["ascii", "utf-8"], chars_min="5")
    data = text_lines(random.Random(3), 300_000)
    plain = sx.Scanner(ms, device=sx.SX_HOST_ONLY)
    monkeypatch.setenv("SX_HOST_MERGE_SEG_BYTES", "20000")
    cutting = sx.Scanner(ms, device=sx.SX_HOST_ONLY)
    try:
        assert n_segments_of_a_host_merge(plain, ms, data) == 1        # set after sx_create: nothing
        n_cut = n_segments_of_a_host_merge(cutting, ms, data)
        assert n_cut > 5
        monkeypatch.delenv("SX_HOST_MERGE_SEG_BYTES")
        plain.reset(); cutting.reset()
        assert n_segments_of_a_host_merge(cutting, ms, data) == n_cut  # removed after sx_create: still cut at that size
        assert n_segments_of_a_host_merge(plain, ms, data) == 1
    finally:
        plain.close(); cutting.close()
