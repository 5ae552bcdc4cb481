#!/usr/bin/env python3
"""Per-kernel VGPRs / LDS / occupancy of one csrc/*.hip (hipcc -Rpass-analysis=kernel-resource-usage; cross-compiles,
no GPU needed), as the tests read them.  python tools/kernel_usage.py lmaze_foveal.hip [name-fragment]"""
import os
import subprocess
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from helpers import kernel_usage  # noqa: E402

if __name__ == "__main__":
    frag = sys.argv[2] if len(sys.argv) > 2 else ""
    for k, v in sorted(kernel_usage(sys.argv[1]).items()):
        if frag in k:
            name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip()
            print("%-90s %s" % (name.split("(")[0][-90:], v))
