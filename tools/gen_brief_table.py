#!/usr/bin/env python3
"""Regenerates csrc/nid_brief_table.hpp: the 256 sample pairs of the upright BRIEF descriptor (nid_match_kernels.hpp k_describe).
Every coordinate lies in [-15, 15].  The draws come from the counter-based splitmix64 generator of the RANSAC sampler
(nid_pose_kernels.hpp pose_mix): draw c = mix(mix(SEED) + c), coordinate = mulhi(draw, 31) - 15, four draws per pair
(ax, ay, bx, by) with the counter running on; a pair whose two samples coincide is drawn again.  Fixed seed: the output is the
same bytes every time (tests/test_matching_host.py compares them with the committed header).
Usage: gen_brief_table.py > direct_visual_lidar_calibration_amd/csrc/nid_brief_table.hpp"""
import sys

SEED = 0x42524945462D3235  # "BRIEF-25"
PAIRS = 256
REACH = 15
MASK = (1 << 64) - 1


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def pairs():
    base, c, out = mix(SEED), 0, []
    while len(out) < PAIRS:
        v = [((mix((base + c + k) & MASK) * (2 * REACH + 1)) >> 64) - REACH for k in range(4)]
        c += 4
        if (v[0], v[1]) != (v[2], v[3]):
            out.append(tuple(v))
    return out


def header():
    lines = ["// nid_brief_table.hpp -- the 256 sample pairs (ax, ay, bx, by), each coordinate in [-15, 15], of the upright BRIEF descriptor",
             "// (tools/gen_brief_table.py: splitmix64, seed 0x%016x; regenerating reproduces this file byte for byte)." % SEED,
             "#pragma once", "namespace nidreg {", "constexpr int kBriefPairs = %d;" % PAIRS, "constexpr int kBriefReach = %d;" % REACH, "#define NID_BRIEF_TABLE_VALUES \\"]
    rows = pairs()
    for i in range(0, PAIRS, 8):
        lines.append("  " + " ".join("%d,%d,%d,%d," % p for p in rows[i:i + 8]) + (" \\" if i + 8 < PAIRS else ""))
    lines.append("}  // namespace nidreg")
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    sys.stdout.write(header())
