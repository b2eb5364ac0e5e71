"""The convolution planners' answers for a fixed list of layer shapes under every afd_debug_conv_path mode, as a table.

Nothing is launched and no GPU is needed: the script only asks the query entry points (afd_conv3x3_weight_kinds,
afd_conv3x3_wino_workspace_bytes, afd_conv_wgrad_form, afd_conv_wgrad_workspace_bytes, afd_conv_wgrad3_plan).  Each mode is
applied from the default state; the table keeps the default state in full and, per mode, only the shapes whose answers differ.

tests/conv_plan_table.json is this script's output and tests/test_conv_plan_table_host.py replays it: a change of the dispatch
code that moves a rule shows there.  Regenerate the file only when a rule is changed on purpose:

    python tools/conv_plan_table.py --out tests/conv_plan_table.json
"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# the modes that return every switch to its default
DEFAULT_MODES = (0, 8, 34, 48, 50, 60, 64, 74, 76, 78, 80, 84, 88, 92, 96, 100000)
# every accepted mode (100007: one value of the Winograd grid family 100000 + g)
MODES = (0, 1, 2, 8, 9, 10, 32, 33, 34, 48, 49) + tuple(range(50, 56)) + tuple(range(59, 64)) + tuple(range(64, 71)) + \
        tuple(range(71, 83)) + (84, 85, 86, 88, 89, 92, 93, 96, 97, 98, 100000, 100007)

# (Cin, Cout, H, W): the 3x3 and 1x1 layer shapes of tests/unet64_cases.py and tests/param_grad_cases.py ...
LAYERS = [
    (64, 64, 64, 64), (64, 96, 64, 64), (128, 64, 64, 64), (8, 32, 64, 64), (3, 64, 64, 64), (16, 64, 64, 64), (64, 32, 64, 64),
    (16, 32, 64, 64), (64, 64, 2, 2), (128, 128, 64, 64), (256, 512, 8, 8), (512, 512, 8, 8), (512, 256, 8, 8), (512, 512, 16, 16),
    (512, 256, 16, 16), (256, 256, 32, 32), (256, 128, 32, 32), (64, 64, 32, 32), (64, 128, 32, 32), (128, 128, 32, 32),
    (128, 64, 32, 32), (128, 128, 16, 16), (128, 256, 16, 16), (256, 256, 16, 16), (256, 128, 16, 16), (256, 256, 8, 8),
    (32, 64, 8, 16), (32, 64, 16, 8), (64, 32, 32, 16), (64, 64, 4, 8),
    (256, 768, 16, 16), (256, 768, 8, 8), (128, 384, 32, 32), (64, 192, 64, 64), (64, 3, 64, 64),
    (3, 32, 32, 32), (64, 64, 16, 16), (128, 128, 8, 8), (64, 96, 4, 4), (12, 40, 8, 8),
    (32, 96, 16, 16), (32, 32, 4, 4), (24, 40, 8, 8), (32, 3, 32, 32), (32, 32, 8, 8),
    # ... and the edges they leave: Cout = 48, the 4x4 maps of the wide layers, a thin 32-channel pair
    (32, 48, 16, 16), (128, 128, 4, 4), (256, 256, 4, 4), (32, 32, 32, 32),
]
BATCHES = (256, 6, 1)
SHAPES = [(B,) + l for B in BATCHES for l in LAYERS]
FIELDS = ("weight_kinds", "wino_ws_fwd", "wino_ws_dgrad", "wgrad_form_k1", "wgrad_form_k3", "wgrad_ws_k1", "wgrad_ws_k3",
          "wgrad3_slabs", "tiles_per_split", "tiles", "block_cout", "block_cin", "waves")


def record(L, shape):
    """the FIELDS of one (B, Cin, Cout, H, W) under the library's current switches"""
    info = (ctypes.c_int * 5)()
    slabs = L.afd_conv_wgrad3_plan(*shape, ctypes.addressof(info))
    return [L.afd_conv3x3_weight_kinds(*shape), L.afd_conv3x3_wino_workspace_bytes(*shape, 0), L.afd_conv3x3_wino_workspace_bytes(*shape, 1),
            L.afd_conv_wgrad_form(*shape, 1), L.afd_conv_wgrad_form(*shape, 3), L.afd_conv_wgrad_workspace_bytes(*shape, 1),
            L.afd_conv_wgrad_workspace_bytes(*shape, 3), slabs] + list(info)


def reset(L):
    for m in DEFAULT_MODES:
        L.afd_debug_conv_path(m)


def sweep(L):
    """-> {"shapes", "fields", "default": one row per shape, "modes": {mode: {shape index: row}} (rows that differ from default)}"""
    reset(L)
    default = [record(L, s) for s in SHAPES]
    modes = {}
    try:
        for m in MODES:
            reset(L)
            L.afd_debug_conv_path(m)
            rows = {str(i): r for i, s in enumerate(SHAPES) for r in [record(L, s)] if r != default[i]}
            modes[str(m)] = rows
    finally:
        reset(L)
    return {"shapes": [list(s) for s in SHAPES], "fields": list(FIELDS), "default": default, "modes": modes}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default=None, help="write the table here (default: print a summary only)")
    a = ap.parse_args()
    import afdm
    t = sweep(afdm.lib())
    for m, rows in t["modes"].items():
        print(f"mode {m}: {len(rows)} of {len(SHAPES)} shapes differ from the default state")
    if a.out:
        with open(a.out, "w") as f:
            json.dump(t, f, separators=(",", ":"))
            f.write("\n")
        print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
