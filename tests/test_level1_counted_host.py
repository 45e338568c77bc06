"""CPU test of the counted level 1's layout arithmetic (csrc/ggd_binning_layout.h: bucket_rows, boundary_rows, total_counted of
ggd_rowbin_tmp): tests/host/l1_counted_layout.cpp -- a stand-alone program that includes nothing else -- is compiled with the
system C++ compiler and -fsanitize=address,undefined and run as a child process, as tests/test_binning_layout_host.py does.
The two row tables lie behind everything the other forms of the row binning use (whose offsets and total keep the parent's
values, restated here), hold GGD_MSD_BINS and rb_blocks1(P) rows of 64 words, overlap nothing and fit total_counted."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_gan_decoder_amd", "csrc")

PS = [1, 1023, 1024, 1025, 4096 * 256 + 1, 1_000_000]
CAPS = [0, 1, 1025, 4_152_095]
GRIDS = [(16, 16), (1024, 1024), (1040, 1024), (4080, 4080)]
CASES = list(itertools.product(PS, CAPS, GRIDS))


def align(v, a=256):
    return (v + a - 1) // a * a


def parent_offsets(P, cap, W, H):
    """the row binning's scratch before the row tables existed (tests/test_binning_layout_host.py::rowbin)"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    blocks1 = (P + 1023) // 1024
    if gx > 64 or gy > 64:
        nby, nbx, bins = 64 * ((gy + 63) // 64), 64 * ((gx + 63) // 64), 256
        tab_words = 2 * (bins + 1) + bins + bins + bins * bins
    else:
        nby = nbx = bins = 64
        tab_words = 130 + 64 * 64 + 64 + 64
    blocks2 = (cap + 1023) // 1024 + bins
    sizes = [align(P * 8), align(blocks1 * nby * 4), align(tab_words * 4), align(cap * 8), align(blocks2 * nbx * 4)]
    return dict(zip(("rb_packed", "rb_counts1", "rb_tab", "rb_ent", "rb_counts2", "rb_total"), itertools.accumulate([0] + sizes)))


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and (shutil.which(c) or os.path.exists(c))), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("layout") / "l1_counted_layout")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "host", "l1_counted_layout.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], input="".join(f"{P} {cap} {W} {H}\n" for P, cap, (W, H) in CASES), capture_output=True, text=True,
                         timeout=120)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    rows = [{kv.split("=")[0]: int(kv.split("=")[1]) for kv in line.split()} for line in res.stdout.splitlines()]
    assert len(rows) == len(CASES)
    return rows


def test_existing_offsets_and_total_keep_their_values(layouts):
    for (P, cap, (W, H)), got in zip(CASES, layouts):
        want = parent_offsets(P, cap, W, H)
        assert {k: got[k] for k in want} == want, (P, cap, W, H)


def test_row_tables_lie_behind_the_total_fit_and_do_not_overlap(layouts):
    for (P, cap, (W, H)), got in zip(CASES, layouts):
        assert got["msd_bins"] == 1024 and got["chunks"] == (P + 1023) // 1024
        bucket_bytes, boundary_bytes = got["msd_bins"] * 64 * 4, got["chunks"] * 64 * 4
        assert got["rb_bucket_rows"] >= got["rb_total"], (P, cap, W, H)                    # behind every other region
        assert got["rb_boundary_rows"] >= got["rb_bucket_rows"] + bucket_bytes, (P, cap, W, H)
        assert got["rb_total_counted"] >= got["rb_boundary_rows"] + boundary_bytes, (P, cap, W, H)
        assert got["rb_bucket_rows"] % 256 == 0 and got["rb_boundary_rows"] % 256 == 0      # 16-byte loads of a row's quarter
        assert got["rb_total_counted"] - got["rb_total"] == align(bucket_bytes) + align(boundary_bytes)   # and nothing else was added
        assert got["touch"] == 1
