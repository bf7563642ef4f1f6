"""mpt_render's command line without a GPU.

tests/golden/cli_refusals.json (tests/golden/make_cli_refusals.py) holds command lines that end before a Renderer exists — refused
combinations, one per arm of every check and pairs that decide their order, flags without a value, unknown flags and words — each with
the exit status, the exact stderr and whether stdout is the usage text, recorded from the binary of the commit before the flag table and
the conflict rows (csrc/host/cli_options.h) replaced the if / else chain: the built binary must answer every one the same.

tests/cli/checkpoint_check.cpp is a stand-alone program over csrc/host/cli_checkpoint.h alone: the four header kinds byte for byte,
every refusal of a --resume with its message, and the write that must not destroy the old file.  Built with the host compiler,
AddressSanitizer and UndefinedBehaviorSanitizer; nothing is loaded into Python."""
import json
import os
import shutil
import subprocess

import pytest

from conftest import GOLDEN, ROOT, scene_path

CLI = os.path.join(ROOT, "metalpathtracer_amd", "lib", "mpt_render")
ROWS = json.load(open(os.path.join(GOLDEN, "cli_refusals.json")))


def run(argv):
    return subprocess.run([CLI] + [a.replace("{scene}", scene_path("scene.xml")) for a in argv], capture_output=True, text=True)


def test_cli_answers_every_recorded_line_as_recorded():
    assert len(ROWS) >= 270 and len({tuple(r["argv"]) for r in ROWS}) == len(ROWS)
    assert all(r["status"] == 2 or (r["status"] == 0 and r["usage"]) for r in ROWS)
    usage = run(["--help"]).stdout
    differ = []
    for row in ROWS:
        r = run(row["argv"])
        if (r.returncode, r.stderr, r.stdout) != (row["status"], row["stderr"], usage if row["usage"] else ""):
            differ.append((row["argv"], row["status"], row["stderr"], r.returncode, r.stderr, r.stdout[:80]))
    assert not differ, "%d of %d lines differ, the first: %r" % (len(differ), len(ROWS), differ[0])


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = str(tmp_path_factory.mktemp("cli") / "checkpoint_check")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I" + os.path.join(ROOT, "metalpathtracer_amd", "csrc", "host"),
                    os.path.join(ROOT, "tests", "cli", "checkpoint_check.cpp"), "-o", exe], check=True)
    return exe


def test_checkpoint_headers_refusals_and_the_safe_write(checker, tmp_path):
    r = subprocess.run([checker, str(tmp_path)], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "all passed" in r.stdout and not r.stderr, r.stdout + r.stderr
    assert sorted(os.listdir(tmp_path)) == ["kept.ck"]   # (what the failed write had to leave, and nothing else)
