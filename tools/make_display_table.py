#!/usr/bin/env python3
"""The encoding thresholds of the display stage (include/mpt.h, "display", step D).

T[k], k = 1..255, is the float32 nearest to f^-1((k - 0.5) / 255), f^-1 the inverse of the transfer function, computed in
float64: a value y encodes to the number of thresholds <= y, which is round(255 f(y)) without a transcendental at run time.

    python tools/make_display_table.py            writes metalpathtracer_amd/csrc/mpt_display_table.h
    python tools/make_display_table.py --check    exits 1 if the committed header differs from what it would write

tests/test_display_cpu.py imports table() and compares it with what mpt_display_table returns.
"""
import os
import sys

import numpy as np

SRGB, GAMMA22, LINEAR = 0, 1, 2
NAMES = ("SRGB", "GAMMA22", "LINEAR")
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metalpathtracer_amd", "csrc", "mpt_display_table.h")


def inverse(transfer, s):
    """f^-1 in float64: the linear value whose encoding is s (0..1)."""
    s = np.asarray(s, np.float64)
    if transfer == SRGB:
        return np.where(s <= 0.04045, s / 12.92, ((s + 0.055) / 1.055) ** 2.4)
    if transfer == GAMMA22:
        return s ** 2.2
    if transfer == LINEAR:
        return s
    raise ValueError("transfer %r" % (transfer,))


def table64(transfer):
    """The 255 thresholds in float64, index 0 = T[1]."""
    k = np.arange(1, 256, dtype=np.float64)
    return inverse(transfer, (k - 0.5) / 255.0)


def table(transfer):
    """The 255 thresholds as committed: float32, index 0 = T[1]."""
    return table64(transfer).astype(np.float32)


def render():
    out = ["// mpt_display_table.h — written by tools/make_display_table.py; do not edit.",
           "// T[k], k = 1..255 (index k - 1): the float32 nearest to f^-1((k - 0.5) / 255) per transfer function (include/mpt.h, display",
           "// step D), as hexadecimal float literals: the compiler reads them exactly.",
           "#pragma once",
           "",
           "static const float MPT_DISPLAY_TABLE[3][255] = {"]
    for t in (SRGB, GAMMA22, LINEAR):
        out.append("    {   // MPT_TRANSFER_%s" % NAMES[t])
        vals = [float(v).hex() + "f" for v in table(t)]
        for i in range(0, 255, 6):
            out.append("        " + ", ".join(vals[i:i + 6]) + ",")
        out.append("    },")
    out.append("};")
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    text = render()
    if "--check" in sys.argv[1:]:
        sys.exit(0 if os.path.exists(HEADER) and open(HEADER).read() == text else 1)
    with open(HEADER, "w") as f:
        f.write(text)
    print("wrote", HEADER)
