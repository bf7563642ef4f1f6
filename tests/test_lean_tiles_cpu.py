"""The per-tile class word of the lean wave-local kernels (lean_tile_class, metalpathtracer_amd/csrc/mpt_lean_tiles.h), on the CPU.

tests/lean_tiles/lean_tiles_check.cpp is a stand-alone program that includes the header.  Soundness: for every `skip` tile of every case,
every pixel of it and the jitters {0, 1 - 2^-24}^2, the four edge midpoints and 4096 random 24-bit pairs, a float32 restatement of the
primary path finds that every chain box misses and every sphere outside the mask is rejected.  Not vacuous: per case the number of tiles
of each class it is meant to have — scene.xml's default view at 70 x 45 has at least a fifth of its 54 tiles `skip` with an empty mask
and at least one with a one-bit mask (both confirmed on the CPU: 18 and 18).  Off switches: a NaN camera or viewport, a camera outside
the shrunk root box, one inside it but outside the tail box, a tree without T, no spheres, a chain of nine nodes (eight are accepted), W or H that the tile counts
do not cover — "general" everywhere.

Built twice with the host compiler, plain and with AddressSanitizer + UndefinedBehaviorSanitizer, and run directly; nothing is loaded
into Python."""
import os
import re
import shutil
import subprocess

import pytest

from conftest import ROOT

SRC = os.path.join(ROOT, "tests", "lean_tiles", "lean_tiles_check.cpp")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc")]
CASES = ("default_70x45", "default_64x64", "horizon_row", "straight_up", "straight_down", "sphere100_in_view", "triangle_in_sky", "chain_of_8")
OFFS = ("nan_camera", "nan_viewport", "camera_outside_tail_box", "camera_outside_root_box", "tree_without_T", "no_spheres", "chain_of_9",
        "size_not_covered", "width_not_whole", "too_few_tile_columns")


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan-ubsan"])
def test_tile_classes_sound_not_vacuous_and_off(tmp_path, sanitize):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path / "lean_tiles_check")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.run([cxx] + FLAGS + extra + [SRC, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all passed" in r.stdout and "FAILED" not in r.stdout, r.stdout + r.stderr
    rows = {m[0]: [int(x) for x in m[1:]] for m in re.findall(
        r"case (\w+): tiles (\d+) general (\d+) sky (\d+) masked (\d+) onebit (\d+) rays (\d+) violations (\d+)", r.stdout)}
    assert sorted(rows) == sorted(CASES)
    for name, (tiles, general, sky, masked, onebit, rays, bad) in rows.items():
        assert bad == 0 and tiles == general + sky + masked and sky + masked > 0, name
        assert rays == (sky + masked) * 64 * (8 + 4096), name
    tiles, general, sky, masked, onebit, _, _ = rows["default_70x45"]
    assert tiles == 54 and 5 * sky >= tiles and onebit >= 1
    offs = {m[0]: (int(m[1]), int(m[2])) for m in re.findall(r"off (\w+): tiles (\d+) general (\d+)", r.stdout)}
    assert sorted(offs) == sorted(OFFS)
    for name, (tiles, general) in offs.items():
        assert tiles > 0 and general == tiles, name
