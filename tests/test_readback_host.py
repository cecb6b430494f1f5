"""The Newton loop's scalar read-back (csrc/readback.hpp) on the host: tests/csrc/readback_check.cpp, a stand-alone program
(its own main, plain g++, -fsanitize=address,undefined) that includes only that header, answers one command per line.

What is pinned here are literal numbers, transcribed from the launchers and consumers as they were before the layout had
names, not read from the header: the slots, the parameters every finishing launch is built with, what the host decodes from
the 16-double block, and the four doubles a sharded problem sums over its ranks for each read-back."""
import math
import os
import struct
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
NAN, INF = float("nan"), float("inf")


def hx(v):
    return struct.pack(">d", float(v)).hex()


def unhx(h):
    return struct.unpack(">d", bytes.fromhex(h))[0]


def block(**slots):
    """16 doubles, slot k = 1000 + k unless given as s<k>=value: a decoder that reads the wrong slot shows."""
    b = [1000.0 + k for k in range(16)]
    for name, v in slots.items():
        b[int(name[1:])] = v
    return " ".join(hx(v) for v in b)


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("readback") / "readback_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, os.path.join(HERE, "csrc", "readback_check.cpp")], check=True, timeout=600)

    def run(*lines):
        r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr
        out = r.stdout.split("\n")[:-1]
        assert len(out) == len(lines)
        return out
    return run


def params(line):
    """'njobs N job BASE OFF COUNT OUT ... out block ints ...' -> (jobs, dict of the rest)"""
    t = line.split()
    assert t[0] == "njobs"
    n, jobs, k = int(t[1]), [], 2
    for _ in range(n):
        assert t[k] == "job"
        jobs.append((t[k + 1], int(t[k + 2]), int(t[k + 3]), int(t[k + 4])))
        k += 5
    rest = dict(zip(t[k::2], t[k + 1::2]))
    return jobs, rest


def test_slot_numbers(ask):
    (line,) = ask("slots")
    t = line.split()
    got = dict(zip(t[::2], map(int, t[1::2])))
    assert got == {"VALUE": 0, "AUX": 1, "SUMSQ": 2, "BAD": 3, "MOVED": 4, "GDOTV": 4, "PIVOT": 5, "LEAF": 6, "STAMP": 15,
                   "SLOTS": 16, "SHARD": 4}


@pytest.mark.parametrize("has_f0", (1, 0))
def test_trial_params(ask, has_f0):
    (line,) = ask(f"trial_params {has_f0} 77 130 9")
    jobs, rest = params(line)
    sums = [("partials", 0, 130, 2), ("partials", 130, 130, 3)]
    assert jobs == ([("f0", 0, 77, 0)] if has_f0 else []) + sums
    assert rest == {"out": "block", "ints": "ints", "nints": "1", "ints_out": "4", "reset": "0", "host": "host", "host_lo": "0",
                    "host_n": "5", "seq": "9"}


def test_direction_params(ask):
    (line,) = ask("dir_params 1000 12")
    jobs, rest = params(line)
    assert jobs == [("partials", 0, 1000, 2), ("partials", 1000, 1000, 3), ("partials", 2000, 1000, 4)]
    assert rest == {"out": "block", "ints": "ints", "nints": "2", "ints_out": "5", "reset": "1", "host": "host", "host_lo": "2",
                    "host_n": "5", "seq": "12"}


def test_plain_params(ask):
    dot0, dot4, stats0, stats2 = ask("plain 1 256 0", "plain 1 3 4", "plain 2 513 0", "plain 2 1 2")
    no_host = {"out": "block", "ints": "null", "nints": "0", "reset": "0", "host": "null", "host_n": "0", "seq": "0"}
    for line, want in ((dot0, [("partials", 0, 256, 0)]), (dot4, [("partials", 0, 3, 4)]),
                       (stats0, [("partials", 0, 513, 0), ("partials", 513, 513, 1)]),
                       (stats2, [("partials", 0, 1, 2), ("partials", 1, 1, 3)])):
        jobs, rest = params(line)
        assert jobs == want
        assert {k: rest[k] for k in no_host} == no_host


@pytest.mark.parametrize("stamp", (1, 5, 2**31 - 1))
def test_decode_trial_moved_only_at_the_stamp(ask, stamp):
    slot4 = [float(stamp - 1), float(stamp), 0.0]
    out = ask(*[f"decode_trial {stamp} " + block(s4=v) for v in slot4])
    for v, line in zip(slot4, out):
        value, sumsq, bad, moved = line.split()
        assert (unhx(value), unhx(sumsq), unhx(bad)) == (1000.0, 1002.0, 1003.0)
        assert int(moved) == (1 if v == float(stamp) else 0), (stamp, v)


def test_decode_trial_passes_values_through(ask):
    cases = [(NAN, 2.5, 0.0), (INF, NAN, 0.0), (-INF, INF, 3.0), (-0.0, 0.0, 1.0), (1.25, -NAN, 7.0)]
    out = ask(*[f"decode_trial 3 " + block(s0=a, s2=b, s3=c, s4=3.0) for a, b, c in cases])
    for (a, b, c), line in zip(cases, out):
        assert line.split() == [hx(a), hx(b), hx(c), "1"]          # bit for bit, NaN payload and sign included


def test_decode_direction(ask):
    flags = [(0.0, 0.0), (1.0, 0.0), (0.0, 2.0), (-3.0, 0.5), (-0.0, NAN), (INF, 1e-300)]
    out = ask(*["decode_dir " + block(s2=NAN, s3=4.0, s4=-INF, s5=p, s6=q) for p, q in flags])
    for (p, q), line in zip(flags, out):
        sumsq, bad, gdotv, pivot, leaf = line.split()
        assert (sumsq, bad, gdotv) == (hx(NAN), hx(4.0), hx(-INF))
        assert (int(pivot), int(leaf)) == (int(p != 0.0), int(q != 0.0))


def left_sum(vals):
    s = vals[0]
    for v in vals[1:]:
        s = s + v
    return s


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or hx(a) == hx(b)


def parse_shard(line, R):
    t = line.split()
    for r in range(R):                                 # every rank's pack wrote exactly 4 doubles, nothing beside them
        assert t[4 * r:4 * r + 4] == ["packed", "4", "guards", "1"]
    t = t[4 * R:]
    assert t[0] == "sums" and t[5] == "record" and len(t[1:5]) == 4
    return [unhx(h) for h in t[1:5]], t[6:]


RANKS = [(0.1, 1e16, 3.0, 0.0), (0.2, -1e16, 1.0, 2.0), (0.3, 1.0, 1e-8, 0.0), (-0.7, 0.5, 0.25, 1.0)]     # value/sumsq, ...


@pytest.mark.parametrize("R", (1, 2, 4))
@pytest.mark.parametrize("movers", ((), (0,), (3,), (0, 1, 2, 3)))
def test_sharded_trial(ask, R, movers):
    stamp = 41
    ranks = RANKS[:R]
    blocks = [block(s0=v, s2=s, s3=b, s4=float(stamp if r in movers else stamp - 1)) for r, (v, s, b, _) in enumerate(ranks)]
    (line,) = ask(f"shard_trial {R} {stamp} " + " ".join(blocks))
    sums, rec = parse_shard(line, R)
    nmoved = len([r for r in movers if r < R])
    want = [left_sum([v for v, _, _, _ in ranks]), float(nmoved), left_sum([s for _, s, _, _ in ranks]), left_sum([b for _, _, b, _ in ranks])]
    assert all(same(a, b) for a, b in zip(sums, want)), (sums, want)          # order: value, moved, sumsq, bad
    assert rec == [hx(want[0]), hx(want[2]), hx(want[3]), str(int(nmoved > 0))]


@pytest.mark.parametrize("R", (1, 2, 4))
@pytest.mark.parametrize("failed", ((), (1,), (2,), (0, 1, 2, 3)))
def test_sharded_direction(ask, R, failed):
    ranks = RANKS[:R]
    # the flags in the block do not travel: the rank's status does (formed from them before the sum)
    blocks = [f"{int(r in failed)} " + block(s2=s, s3=b, s4=g, s5=float(r % 2), s6=7.0) for r, (g, s, b, _) in enumerate(ranks)]
    (line,) = ask(f"shard_dir {R} " + " ".join(blocks))
    sums, rec = parse_shard(line, R)
    nfailed = len([r for r in failed if r < R])
    want = [left_sum([s for _, s, _, _ in ranks]), left_sum([b for _, _, b, _ in ranks]), left_sum([g for g, _, _, _ in ranks]), float(nfailed)]
    assert all(same(a, b) for a, b in zip(sums, want)), (sums, want)          # order: sumsq, bad, gdotv, status
    assert rec == [hx(want[0]), hx(want[1]), hx(want[2]), "failed", str(int(nfailed > 0))]


def test_sharded_sums_carry_non_finite_values(ask):
    (line,) = ask("shard_trial 2 1 " + block(s0=INF, s2=NAN, s3=1.0, s4=1.0) + " " + block(s0=1.0, s2=1.0, s3=0.0, s4=0.0))
    sums, rec = parse_shard(line, 2)
    assert sums[0] == INF and sums[1] == 1.0 and math.isnan(sums[2]) and sums[3] == 1.0
    assert rec[0] == hx(INF) and math.isnan(unhx(rec[1])) and rec[2:] == [hx(1.0), "1"]
