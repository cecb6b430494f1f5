"""Threads per front of an mf_factor_small launch (csrc/mf_launch_plan.hpp: factor_small_threads), on the host:
tests/csrc/small_threads_check.cpp, a stand-alone program (its own main, plain g++, -fsanitize=address,undefined), prints the
rule for every class, every count up to ten fronts per compute unit, 1 / 104 / 256 compute units and every forced value.

What is pinned here is the rule as DESIGN.md section 4 states it, transcribed independently: with per_cu = ceil(count / CU)
workgroups of the launch on a compute unit, at most what the class's LDS lets it hold at a time, the widest of 256 / 512 /
1024 threads with per_cu * threads / 64 <= 24 waves; 64 / 128 for the classes 16 / 32 whatever is forced.
The sixteen-small-children branch of the kernel runs on the first four waves of any wider workgroup, so no launch is forced
back to 256 threads on its account."""
import collections
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CLASSES = (16, 32, 48, 64, 88, 128)
CUS = (1, 104, 256)
FORCED = (0, 256, 512, 1024, 300)          # 300: not a size, ignored
CU_LDS, STATIC_LDS, FILL_WAVES = 160 * 1024, 2112, 24


def lds_bytes(cls):
    return 8 * ((cls * (cls + 1) // 2 if cls >= 88 else cls * cls) + 8 * cls)


def model(cls, cu, forced, count):
    if cls <= 16:
        return 64
    if cls <= 32:
        return 128
    if forced in (256, 512, 1024):
        return forced
    per_cu = min(-(-count // cu), CU_LDS // (lds_bytes(cls) + STATIC_LDS))
    return max(t for t in (256, 512, 1024) if t == 256 or per_cu * t // 64 <= FILL_WAVES)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("small_threads") / "small_threads_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "small_threads_check.cpp")], check=True, timeout=600)
    r = subprocess.run([exe] + [str(c) for c in CUS], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
    t = collections.defaultdict(dict)
    for line in r.stdout.split("\n"):
        if line:
            cls, cu, forced, count, threads, lds = map(int, line.split())
            assert lds == lds_bytes(cls)
            t[cls, cu, forced][count] = threads
    return t


def test_every_class_width_and_forced_value_is_there(table):
    assert set(table) == {(c, u, f) for c in CLASSES for u in CUS for f in FORCED}
    for (cls, cu, forced), row in table.items():
        assert sorted(row) == list(range(1, 10 * cu + 3))


def test_only_allowed_sizes_and_enough_threads_for_the_panel_rows(table):
    for (cls, cu, forced), row in table.items():
        allowed = {64} if cls <= 16 else ({128} if cls <= 32 else {256, 512, 1024})
        assert set(row.values()) <= allowed, (cls, cu, forced)
        assert min(row.values()) >= cls - 1


def test_forced_sizes_hold_for_the_classes_above_32_only(table):
    for (cls, cu, forced), row in table.items():
        if forced in (256, 512, 1024) and cls > 32:
            assert set(row.values()) == {forced}, (cls, cu, forced)
        if forced == 300:
            assert row == table[cls, cu, 0], (cls, cu)


def test_rule_is_monotone_in_the_count(table):
    for (cls, cu, forced), row in table.items():
        seq = [row[c] for c in sorted(row)]
        assert all(a >= b for a, b in zip(seq, seq[1:])), (cls, cu, forced)


def test_rule_is_the_stated_one_at_every_count(table):
    for (cls, cu, forced), row in table.items():
        for count, threads in row.items():
            assert threads == model(cls, cu, forced, count), (cls, cu, forced, count, threads)


@pytest.mark.parametrize("cu", CUS)
def test_thresholds_sit_where_the_measurements_put_them(table, cu):
    """Just below and above each threshold: 1024 threads up to one front per compute unit, 512 up to three, 256 from there on
    and for every launch that fills the device -- except class 128, whose LDS lets a compute unit hold two fronts at a time,
    whatever the count: 512 from two fronts per compute unit on."""
    for cls in (48, 64, 88, 128):
        row = table[cls, cu, 0]
        assert row[1] == row[cu] == 1024 and row[cu + 1] == 512, (cls, cu)
        assert row[3 * cu] == 512, (cls, cu)
        assert row[3 * cu + 1] == row[10 * cu + 2] == (512 if cls == 128 else 256), (cls, cu)
