"""Generates the ``TURBO`` literal of direct_visual_lidar_calibration_amd/draw.py: 256 x 3 uint8,
``trunc(255 * matplotlib.colormaps["turbo"](i)[:3])`` for integer i (an integer argument indexes the colour map's 256-entry table
directly) -- the colours the reference's matcher script gives its match lines (scripts/find_matches_superglue.py), as RGB.

    python tools/make_turbo_table.py            print the literal
    python tools/make_turbo_table.py --write    replace the block between the TURBO markers of draw.py
    python tools/make_turbo_table.py --check    exit 1 unless draw.py holds exactly this table

matplotlib is needed here only: nothing at run time imports it (tests/test_draw_host.py compares the two where it is installed).
"""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRAW = os.path.join(ROOT, "direct_visual_lidar_calibration_amd", "draw.py")
BEGIN, END = "# TURBO-BEGIN (tools/make_turbo_table.py)\n", "# TURBO-END\n"


def table():
    import matplotlib

    cmap = matplotlib.colormaps["turbo"]
    return [tuple(int(255 * c) for c in cmap(i)[:3]) for i in range(256)]


def literal(rows):
    lines = ["TURBO = np.array(["]
    for k in range(0, 256, 8):
        lines.append("    " + " ".join("(%d, %d, %d)," % r for r in rows[k:k + 8]))
    lines.append("], dtype=np.uint8)")
    return "\n".join(lines) + "\n"


def main(argv):
    text = literal(table())
    if "--write" in argv or "--check" in argv:
        src = open(DRAW).read()
        m = re.search(re.escape(BEGIN) + r"(.*?)" + re.escape(END), src, flags=re.S)
        if not m:
            raise SystemExit(f"{DRAW}: TURBO markers not found")
        if "--check" in argv:
            return 0 if m.group(1) == text else 1
        with open(DRAW, "w") as f:
            f.write(src[:m.start(1)] + text + src[m.end(1):])
        return 0
    sys.stdout.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
