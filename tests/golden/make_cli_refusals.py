"""Records tests/golden/cli_refusals.json: what an mpt_render binary answers to the command lines it ends before a Renderer exists.

For each argument vector below ({scene} stands for assets/scene.xml) the file keeps the exit status, the exact stderr and whether stdout
is the usage text, which is compared with the same binary's --help output and not stored.  tests/test_cli_cpu.py replays the file
against the built binary.  The committed file was recorded from the binary of commit 14bbba7, the last one whose main.cpp parsed the
flags in an if / else chain and refused combinations in hand-written ladders: the order of those ladders and of their arms decides
which message a command line with several faults gets, and that order is behaviour.

Run:  python tests/golden/make_cli_refusals.py path/to/mpt_render
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(os.path.dirname(os.path.dirname(HERE)), "assets", "scene.xml")

S = ["--scene", "{scene}"]
PPM = S + ["--out", "x.ppm"]
PATH = ["--camera-path", "p.txt"]
# what the plain-run modes (--ao, --direct) meet, in the order of --ao's ladder; --direct's has --ao after the .ppm arm
PLAIN_ONLY = [["--frames", "2"], PATH, ["--gpus", "2"], ["--adaptive", "0.05"], ["--denoise"], ["--tonemap", "aces"], ["--exposure", "1"], ["--white", "2"],
              ["--auto-exposure"], ["--transfer", "linear"], ["--temporal"], ["--svgf"], ["--checkpoint", "c.sum"], ["--resume", "c.sum"]]


def cases():
    c = []
    # ---- the argument lists of the existing refusal tests (test_adaptive_cpu, test_temporal_cpu, test_svgf_cpu, the `bad` lists of
    #      test_gpu_ao, _direct, _nee, _nee_adaptive, _cone, _ris, _restir, _display), with their files' names shortened
    for extra in (["--frames", "2"], ["--gpus", "2"], ["--rng", "literal"], ["--checkpoint", "x.sum"], ["--resume", "x.sum"], PATH):
        c.append(S + ["--adaptive", "0.05"] + extra)
    for extra in ([], PATH + ["--rng", "literal"], PATH + ["--gpus", "2"], PATH + ["--checkpoint", "x.sum"], PATH + ["--resume", "x.sum"],
                  PATH + ["--temporal-spp", "0"], ["--adaptive", "0.05"] + PATH):
        c.append(S + ["--temporal"] + extra)
    for extra in ([], PATH + ["--temporal"], PATH + ["--denoise"], PATH + ["--rng", "literal"], PATH + ["--gpus", "2"], PATH + ["--checkpoint", "x.sum"],
                  PATH + ["--resume", "x.sum"], PATH + ["--temporal-spp", "0"], ["--adaptive", "0.05"] + PATH, ["--adaptive", "0.05"],
                  PATH + ["--svgf-iterations", "9"], PATH + ["--svgf-iterations", "-1"], PATH + ["--svgf-iterations", "100"]):
        c.append(S + ["--svgf"] + extra)
    gpu_base = S + ["--width", "64", "--height", "48", "--spp", "4", "--depth", "8", "--seed", "1", "--bvh", "reference"]
    a = ["--out", "a.ppm"]
    for bad in (["--out", "c.pfm", "--ao", "8"], a + ["--ao", "0"], a + ["--ao", "8", "--denoise"], a + ["--ao-radius", "1"],
                ["--out", "c.pfm", "--direct", "8"], a + ["--direct", "0"], a + ["--direct", "8", "--denoise"], a + ["--direct", "8", "--ao", "4"],
                a + ["--direct", "8", "--adaptive", "0.05"], a + ["--direct", "8", "--temporal"], a + ["--direct", "8", "--svgf"], a + ["--direct-walk", "own"],
                ["--out", "c.pfm", "--tonemap", "aces"]):
        c.append(gpu_base + bad)
    x = ["--out", "x.ppm"]
    for bad in (["--nee", "--adaptive", "0.05"], ["--nee", "--gpus", "2"], ["--nee", "--ao", "4"], ["--nee", "--direct", "4"], ["--nee", "--rng", "literal"],
                ["--nee", "--bsdf", "scatter-all"], ["--nee", "--frames", "2"], ["--nee-walk", "own"], ["--nee-clamp", "2"], ["--nee"] + PATH,
                ["--nee"] + PATH + ["--temporal"],
                ["--light-sampling", "cone"], ["--light-sampling", "area"], ["--nee", "--light-sampling", "sphere"], ["--light-sampling", "cone", "--ao", "4"],
                ["--light-candidates", "4"], ["--light-candidates", "4", "--ao", "4"], ["--nee", "--light-candidates", "0"], ["--nee", "--light-candidates", "33"],
                ["--direct", "4", "--light-candidates", "-2"], ["--nee-adaptive", "0.05", "--light-candidates", "2"],
                ["--restir", "4"], ["--nee", "--restir", "4"], ["--direct", "4", "--restir-radius", "4"], ["--direct", "4", "--restir-biased"],
                ["--direct", "4", "--restir", "17"], ["--direct", "4", "--restir", "-1"], ["--direct", "4", "--restir", "4", "--restir-radius", "0"],
                ["--direct", "4", "--restir", "4", "--restir-radius", "65"], ["--direct", "4", "--restir", "4", "--light-sampling", "cone"]):
        c.append(gpu_base + x + bad)
    for extra in (["--nee"], ["--adaptive", "0.05"], ["--gpus", "2"], PATH, ["--frames", "2"], ["--checkpoint", "c.sum"], ["--resume", "c.sum"], ["--ao", "4"],
                  ["--direct", "4"], ["--rng", "literal"]):
        c.append(gpu_base + ["--nee-adaptive", "0.1", "--out", "x.pfm"] + extra)
    c.append(gpu_base + ["--nee", "--adaptive", "0.05", "--out", "x.pfm"])

    # ---- one line per arm of every ladder, in the ladder's order
    c.append([])                                                       # no --scene
    for flag in (["--tonemap", "aces"], ["--transfer", "linear"], ["--exposure", "1"], ["--white", "2"], ["--auto-exposure"]):
        c.append(S + ["--out", "x.pfm"] + flag)                        # a display flag needs a .ppm
    for flag in (["--key", "0.2"], ["--percentile", "40"], ["--adaptation", "0.5"]):
        c.append(PPM + flag)                                           # ... go with --auto-exposure
    for extra in (["--nee"], ["--adaptive", "0.05"], ["--nee-clamp", "nan"], ["--gpus", "2"], ["--devices", "0,1"], PATH, ["--frames", "2"], ["--checkpoint", "c.sum"],
                  ["--resume", "c.sum"], ["--ao", "4"], ["--ao-radius", "1"], ["--direct", "4"], ["--direct-walk", "own"], ["--rng", "literal"],
                  ["--bsdf", "scatter-all"]):
        c.append(S + ["--nee-adaptive", "0.1"] + extra)
    c += [S + ["--light-sampling", "cone"], S + ["--light-candidates", "4"], S + ["--nee-adaptive", "0.1", "--light-candidates", "2"]]
    for extra in (["--restir-radius", "4"], ["--restir-biased"], ["--restir", "4"], ["--direct", "4", "--restir", "17"], ["--direct", "4", "--restir", "-1"],
                  ["--direct", "4", "--restir", "4", "--restir-radius", "0"], ["--direct", "4", "--restir", "4", "--restir-radius", "65"],
                  ["--direct", "4", "--restir", "0", "--light-sampling", "cone"]):
        c.append(PPM + extra)
    for extra in (["--nee-walk", "own"], ["--nee-clamp", "2"], ["--nee", "--nee-clamp", "nan"], ["--nee", "--adaptive", "0.05"], ["--nee", "--gpus", "2"],
                  ["--nee"] + PATH, ["--nee", "--frames", "2"], ["--nee", "--ao", "4"], ["--nee", "--ao-radius", "1"], ["--nee", "--direct", "4"],
                  ["--nee", "--direct-walk", "own"], ["--nee", "--rng", "literal"], ["--nee", "--bsdf", "scatter-all"]):
        c.append(S + extra)
    for mode, other in (("--direct", ["--ao", "4"]), ("--ao", None)):
        c += [PPM + [mode, "0"], PPM + [mode, "1025"], PPM + [mode, "x"], S + [mode, "4"], S + ["--out", "x.pfm", mode, "4"]]
        c.append(PPM + [mode + ("-walk" if other else "-radius"), "1"])
        if other:
            c += [PPM + [mode, "4"] + other, PPM + [mode, "4", "--ao-radius", "1"]]
        for extra in PLAIN_ONLY:
            c.append(PPM + [mode, "4"] + extra)
    for extra in (["--frames", "2"], PATH, ["--gpus", "2"], ["--devices", "2,3"], ["--rng", "literal"], ["--checkpoint", "c.sum"], ["--resume", "c.sum"]):
        c.append(S + ["--adaptive", "0.05"] + extra)
    c.append(S + ["--temporal"] + PATH + ["--devices", "0,1"])

    # ---- pairs that decide an order: two faults at once
    c += [["--light-candidates", "0"], ["--light-sampling", "sphere"], ["--nee", "--adaptive", "0.05"],                     # parse-time refusals beat a missing --scene,
          ["--light-candidates", "0", "--light-sampling", "sphere"], ["--light-sampling", "sphere", "--light-candidates", "0"],   # a conflict does not; the first one wins
          S + ["--out", "x.pfm", "--tonemap", "aces", "--key", "0.2"], S + ["--out", "x.pfm", "--tonemap", "aces", "--nee", "--adaptive", "0.05"],
          S + ["--key", "0.2", "--nee-adaptive", "0.1", "--nee"], PPM + ["--key", "0.2", "--exposure", "1", "--ao", "0"],
          S + ["--nee-adaptive", "0.1", "--light-sampling", "cone", "--frames", "2"], S + ["--nee-adaptive", "0.1", "--restir", "4"],
          S + ["--nee-adaptive", "0.1", "--frames", "2"] + PATH, S + ["--nee-adaptive", "0.1", "--resume", "c", "--checkpoint", "c"],
          S + ["--light-sampling", "cone", "--light-candidates", "4"], S + ["--light-candidates", "4", "--restir", "4"],
          S + ["--nee", "--restir", "4", "--adaptive", "0.05"], S + ["--nee", "--light-candidates", "4", "--restir", "4", "--frames", "2"],
          PPM + ["--nee", "--direct", "4"], PPM + ["--nee", "--direct", "0", "--ao", "0"], PPM + ["--nee-walk", "own", "--direct", "0"],
          PPM + ["--nee", "--frames", "2"] + PATH, PPM + ["--nee", "--adaptive", "0.05", "--nee-clamp", "nan"],
          PPM + ["--direct", "4", "--ao", "4"], PPM + ["--direct", "4", "--ao", "0"], PPM + ["--direct", "0", "--ao", "4"],
          PPM + ["--direct", "4", "--frames", "2"] + PATH, PPM + ["--direct", "4", "--resume", "c", "--checkpoint", "c"], PPM + ["--direct", "4", "--svgf", "--temporal"],
          PPM + ["--direct", "4", "--denoise", "--adaptive", "0.05"], S + ["--out", "x.pfm", "--direct", "4", "--tonemap", "aces"],
          PPM + ["--ao", "4", "--adaptive", "0.05", "--frames", "2"], PPM + ["--ao", "4", "--gpus", "2"] + PATH, PPM + ["--ao", "4", "--tonemap", "aces", "--denoise"],
          S + ["--adaptive", "0.05", "--temporal", "--svgf"], S + ["--adaptive", "0.05", "--temporal"] + PATH, S + ["--adaptive", "0.05", "--rng", "literal", "--gpus", "2"],
          S + ["--temporal", "--svgf"], S + ["--temporal", "--svgf"] + PATH, S + ["--temporal", "--temporal-spp", "0", "--resume", "c"] + PATH,
          S + ["--svgf", "--denoise", "--rng", "literal"] + PATH, S + ["--svgf", "--svgf-iterations", "9", "--temporal-spp", "0"] + PATH,
          S + ["--svgf", "--svgf-iterations", "9"], S + ["--devices", "3", "--gpus", "2", "--adaptive", "0.05", "--frames", "1"],
          S + ["--adaptive", "0.05", "--nee-adaptive", "0.1"], S + ["--nee-adaptive", "0.1", "--adaptive", "0.05", "--nee"]]

    # ---- the parser: a flag without its value, an unknown flag, --help, word lists, malformed values
    c += [["--help"], S + ["--help"], ["--help", "--bogus"], ["--bogus", "--help"], ["--bogus"], S + ["--bogus"], S + ["-h"], S + ["scene.xml"],
          S + ["--tonemap", "bogus", "--help"], S + ["--light-candidates", "0", "--help"], S + ["--help", "--light-candidates", "0"]]
    for flag in ("--scene", "--spp", "--seed", "--vfov", "--devices", "--bvh", "--direct-walk", "--tonemap", "--exposure", "--camera-pos", "--light-sampling",
                 "--light-candidates", "--adaptive", "--nee-adaptive", "--resume"):
        c.append(S + [flag])
    c += [S + ["--tonemap", "bogus"], S + ["--transfer", "bogus"], S + ["--tonemap", "srgb"], S + ["--transfer", "aces"], S + ["--light-sampling", "bogus"],
          S + ["--light-sampling", ""], S + ["--light-candidates", "x"],
          # the words that fall back silently do not end the run: each rides on a refusal that would read otherwise had the word been taken
          S + ["--adaptive", "0.05", "--rng", "bogus", "--checkpoint", "c"], S + ["--adaptive", "0.05", "--rng", "philox", "--checkpoint", "c"],
          S + ["--nee", "--bsdf", "bogus", "--ao", "0"], S + ["--nee", "--bsdf", "scatter", "--ao", "0"], S + ["--nee", "--bsdf", "lambert", "--ao", "0"],
          PPM + ["--direct", "0", "--direct-walk", "bogus"], S + ["--nee-walk", "bogus"], PPM + ["--ao", "0", "--bvh", "bogus"], PPM + ["--ao", "0", "--pipeline", "bogus"],
          PPM + ["--ao", "0", "--bvh", "binned", "--pipeline", "ordered"],
          S + ["--devices", "a"], S + ["--devices", "0,-1"], S + ["--devices", "0,,1"], S + ["--devices", "", "--adaptive", "0.05", "--frames", "1"],
          S + ["--devices", "0", "--devices", "1", "--adaptive", "0.05"], S + ["--devices", "0,1,", "--adaptive", "0.05"],
          S + ["--camera-pos", "1,2"], S + ["--camera-dir", "x"], S + ["--camera-up", "1;2;3"], PPM + ["--camera-pos", "1,2,3,4", "--ao", "0"],
          PPM + ["--spp", "x", "--ao", "x"], PPM + ["--direct", "4x", "--frames", "2"], PPM + ["--ao", "4", "--frames", "x", "--gpus", "x", "--denoise"]]
    return c


def record(binary):
    run = lambda argv: subprocess.run([binary] + [a.replace("{scene}", SCENE) for a in argv], capture_output=True, text=True)
    usage = run(["--help"]).stdout
    assert usage.startswith("mpt_render --scene")
    rows, seen = [], set()
    for argv in cases():
        if tuple(argv) in seen:
            continue
        seen.add(tuple(argv))
        r = run(argv)
        assert r.stdout in ("", usage) and (r.returncode == 2 or (r.returncode == 0 and r.stdout == usage)), (argv, r.returncode, r.stdout[:200], r.stderr)
        assert SCENE not in r.stderr, argv
        rows.append({"argv": argv, "status": r.returncode, "stderr": r.stderr, "usage": r.stdout == usage})
    return rows


if __name__ == "__main__":
    rows = record(sys.argv[1])
    with open(os.path.join(HERE, "cli_refusals.json"), "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")
    print("%d command lines" % len(rows))
