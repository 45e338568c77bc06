"""CPU test of the forward's cross-frame speculation policy (csrc/ggd_spec.h): tests/host/spec_trace.cpp -- a stand-alone program
that includes nothing else -- is compiled with the system C++ compiler and -fsanitize=address,undefined and fed scripted frame
reports as a child process.  The expected traces are read off the host code the policy was lifted from (forward_spec_collect,
geometry_enqueue and render_enqueue of ggd_capi.hip); the GPU suite pins the same state machine through the library's counters."""
import os
import shutil
import subprocess

import pytest

from _util import msd_window

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_gan_decoder_amd", "csrc")
EMPTY = (0xffffffff, 0)                       # kmin > kmax: nothing was kept
NARROW = [(0x3fe00000 + 0x1000 * i, 0x3fe80000 + 0x800 * i) for i in range(8)]   # depths around 1.75 .. 1.82
COLS = ("msd", "lo", "shift", "three", "again", "reruns", "msd_frames", "flat_streak", "pause")


@pytest.fixture(scope="module")
def spec_trace(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and (shutil.which(c) or os.path.exists(c))), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("spec") / "spec_trace")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "host", "spec_trace.cpp"), "-o", exe], check=True)

    def run(lines):
        res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and res.stderr == "", res.stderr
        return [dict(zip(COLS, map(int, l.split()))) for l in res.stdout.splitlines()]
    return run


def frame(rng, folded=1, flat=1, ok=0, flags=0, abandoned=0):
    return f"frame {folded} {flat} {ok} {rng[0]} {rng[1]} {flags} {abandoned}"


def test_header_includes_only_stdint():
    src = open(os.path.join(CSRC, "ggd_spec.h")).read()
    assert [l.split()[1] for l in src.splitlines() if l.startswith("#include")] == ["<stdint.h>"]


@pytest.mark.parametrize("name,base", [
    ("narrow", (0x3fe00000, 0x3fe80000)),
    ("straddles the key of 2.0f", (0x3ff00000, 0x40100000)),
    ("margin below 0", (100, 5000)),
    ("margin past 0xfffffffe", (0xfffff000, 0xfffffff0)),
    ("too wide", (0x3f000000, 0x41000000)),
])
def test_warm_up_and_window(spec_trace, name, base):
    ranges = [(base[0] + 7 * i, base[1] + i) for i in range(8)]
    want = msd_window(ranges)
    assert (want is None) == (name == "too wide")
    assert name != "margin below 0" or want[0] == 0
    out = spec_trace([frame(r) for r in ranges] + [frame(base, ok=1)])
    assert [o["msd"] for o in out[:8]] == [0] * 8 and [o["three"] for o in out[:8]] == [0] * 8
    assert [o["flat_streak"] for o in out] == list(range(1, 10))
    ninth = out[8]
    if want is None:    # shift > 16: no plan; the flat streak of eight picks three passes instead
        assert (ninth["msd"], ninth["three"], ninth["msd_frames"]) == (0, 1, 0)
    else:
        assert (ninth["msd"], ninth["lo"], ninth["shift"]) == (1,) + want
        assert (ninth["three"], ninth["again"], ninth["msd_frames"], ninth["reruns"]) == (0, 0, 1, 0)


def test_key_outside_the_window(spec_trace):
    outlier = (0x3f900000, 0x3fe80000)
    fed = NARROW + [NARROW[0], outlier, NARROW[1], NARROW[2]]
    out = spec_trace([frame(r) for r in NARROW] + [frame(NARROW[0], ok=1), frame(outlier, ok=0, flags=4)] +
                     [frame(NARROW[1]), frame(NARROW[2]), frame(NARROW[3], ok=1)])
    miss = out[9]
    assert (miss["msd"], miss["again"], miss["reruns"], miss["msd_frames"], miss["pause"]) == (1, 1, 1, 1, 2)
    assert [o["msd"] for o in out[10:12]] == [0, 0] and [o["pause"] for o in out[10:12]] == [1, 0]
    back = out[12]
    assert (back["msd"], back["lo"], back["shift"]) == (1,) + msd_window(fed)     # the outlier's range has joined the window
    assert (back["again"], back["reruns"], back["msd_frames"]) == (0, 1, 2)


def test_abandoned_frame_counts_no_rerun(spec_trace):
    """forward_spec_collect returns GGD_E_CAPACITY before it counts a rerun: the policy's state moves, the counter does not"""
    out = spec_trace([frame(r) for r in NARROW] + [frame((0x3f900000, 0x3fe80000), ok=0, flags=4, abandoned=1)])
    assert (out[8]["msd"], out[8]["again"], out[8]["reruns"], out[8]["pause"]) == (1, 0, 0, 2)


def test_consecutive_oversized_buckets(spec_trace):
    lines, checks, k = [frame(r) for r in NARROW], [], 0     # checks: (frame index, expected columns)
    rng = lambda: (0x3fa00000 + 0x100 * k, 0x3fa40000 + 0x100 * k)     # below NARROW: a window that still held NARROW would show it
    for n_miss, pause in enumerate((8, 16, 32, 64, 64), 1):
        k += 1
        since = [rng()]                                        # the ring restarts from the missing frame's own range
        checks.append((len(lines), dict(msd=1, again=1, reruns=n_miss, pause=pause, msd_frames=0)))
        lines.append(frame(since[0], ok=0, flags=0))
        for left in range(pause - 1, -1, -1):
            k += 1
            since.append(rng())
            checks.append((len(lines), dict(msd=0, again=0, pause=left)))
            lines.append(frame(since[-1]))
        lo, shift = msd_window(since[-32:])
        checks.append((len(lines), dict(msd=1, lo=lo, shift=shift)))   # (the next round's miss, or the success below)
    k += 1
    lines += [frame(rng(), ok=1), frame(rng(), ok=0, flags=0)]
    checks.append((len(lines) - 2, dict(msd=1, again=0, msd_frames=1, reruns=5)))
    checks.append((len(lines) - 1, dict(msd=1, again=1, reruns=6, pause=8)))     # one success has reset the doubling
    out = spec_trace(lines)
    assert len(out) == len(lines)
    for i, want in checks:
        assert {c: out[i][c] for c in want} == want, (i, out[i])


def test_flat_streak_and_three_passes(spec_trace):
    lines = [frame(r) for r in NARROW] + [frame(NARROW[0], ok=1)]       # default options: the two-launch sort wins at a streak of 8
    out = spec_trace(lines)
    assert [o["three"] for o in out] == [0] * 9 and out[8]["msd"] == 1 and out[7]["flat_streak"] == 8
    lines = (["opts 1 0 1"] + [frame(r) for r in NARROW[:3]] + [frame(NARROW[3], flat=0)] + [frame(r) for r in NARROW] +
             [frame(NARROW[0]), frame(EMPTY, folded=0, flat=0), frame(NARROW[1], flat=0), frame(NARROW[2]), frame(NARROW[3])])
    out = spec_trace(lines)
    assert [o["flat_streak"] for o in out] == [1, 2, 3, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 9, 0, 1, 2]   # a frame that is not folded: no change
    assert [o["three"] for o in out] == [0] * 12 + [1, 0, 1, 0, 0]
    assert [o["again"] for o in out] == [0] * 14 + [1, 0, 0] and [o["reruns"] for o in out] == [0] * 14 + [1, 1, 1]
    assert all(o["msd"] == 0 and o["msd_frames"] == 0 for o in out)
    out = spec_trace(["opts 0 0 1"] + [frame(r) for r in NARROW] + [frame(NARROW[0])])                # GGD_OPT_FOLD must be 1
    assert [o["three"] for o in out] == [0] * 9


def test_empty_frame_leaves_the_ring_alone(spec_trace):
    out = spec_trace([frame(r) for r in NARROW[:7]] + [frame(EMPTY), frame(NARROW[7]), frame(NARROW[0], ok=1)])
    assert [o["msd"] for o in out] == [0] * 9 + [1]
    assert (out[9]["lo"], out[9]["shift"]) == msd_window(NARROW)


def test_reset_restores_warm_up_and_keeps_counters(spec_trace):
    other = [(0x40200000 + 0x1000 * i, 0x40280000 + 0x1000 * i) for i in range(8)]
    out = spec_trace([frame(r) for r in NARROW] + [frame(NARROW[0], ok=1), frame((0x3f900000, 0x3fe80000), ok=0, flags=4), "reset"] +
                     [frame(r) for r in other] + [frame(other[0], ok=1)])
    assert (out[9]["reruns"], out[9]["msd_frames"], out[9]["pause"]) == (1, 1, 2)
    after = out[10:]
    assert [o["msd"] for o in after] == [0] * 8 + [1] and [o["three"] for o in after] == [0] * 9
    assert [o["flat_streak"] for o in after] == list(range(1, 10)) and [o["pause"] for o in after] == [0] * 9
    assert all((o["reruns"], o["msd_frames"]) == (1, 1) for o in after[:8]) and (after[8]["reruns"], after[8]["msd_frames"]) == (1, 2)
    assert (after[8]["lo"], after[8]["shift"]) == msd_window(other)      # nothing of the ranges from before the reset
