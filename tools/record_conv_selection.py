"""Table of the conv kernel selection (host code only, no GPU): what the library answers for every conv shape the models launch, under
every dev switch of the f16x3 choice.  tests/test_conv_selection_host.py compares the library against tests/golden/conv_selection.json.

usage: python tools/record_conv_selection.py OUT.json     records the table from the library this checkout loads (MPHIP_LIB overrides).
       python tools/record_conv_selection.py --show FILE  prints a recorded table, one row per (setting, shape), tab-separated.
The committed table was recorded from the commit BEFORE the planner was unified, plus a patch that adds only mphip_debug_conv3d_plan
written on that commit's scattered conditions — never from the code under test.

Some switches are fixed at first use, so every setting runs in a fresh child process (`--child NAME` prints that setting's rows).
File layout: see dump().
"""
import base64, ctypes, json, lzma, os, subprocess, sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("MPHIP_LIB", os.path.join(ROOT, "megaportrait-hack_amd", "libmphip.so"))
GROUPS = 32
BATCHES = (1, 2, 3, 4, 5, 8)
PLAN_FIELDS = ("kernel", "tile_d", "tile_h", "tile_w", "gn_rows", "tile_list", "max_gn_ci", "splits", "chunks_per_split", "grid_x", "grid_y", "grid_z")
PER_KP = ("supported", "kernel_variant", "splits", "workspace_bytes", "gn_workspace_bytes", "roi_granule", "roi_tile_d", "roi_tile_h",
          "roi_tile_w", "roi_workspace_bytes", "packed_weight_bytes")
KP = ((1, 0), (1, 1), (3, 0), (3, 1))   # (k, precision)
COLUMNS = [f"k{k}p{p}.{c}" for k, p in KP for c in PER_KP] + [f"plan_roi{r}.{c}" for r in (0, 1) for c in ("found",) + PLAN_FIELDS]


def layers():
    """(Ci, Co, D, H, W) of every conv the models launch (per frame), plus shapes off the f16x3 tiling."""
    out = []
    for d, h, w in ((16, 64, 64), (16, 32, 32), (8, 16, 16)):   # G3d on the hot slice's volume (two smaller ones: tests, smoke)
        for lv in range(4):
            c, dims = 96 << lv, (d >> lv, h >> lv, w >> lv)
            out.append((c, c) + dims)                       # conv2 of a down block, the final conv, Eapp's 3-D tail (level 0)
            if lv:
                out.append((c // 2, c) + dims)              # down block: conv1 and its k = 1 shortcut
                out.append((c, c // 2) + dims)              # up block: conv1 and its k = 1 shortcut
                out.append((c // 2, c // 2) + dims)         # up block: conv2
    for ci, co, dims in ((512, 256, (4, 1, 1)), (256, 256, (4, 1, 1)), (256, 128, (8, 2, 2)), (128, 128, (8, 2, 2)), (128, 64, (16, 4, 4)),
                         (64, 64, (16, 4, 4)), (64, 32, (16, 8, 8)), (32, 32, (16, 8, 8)), (32, 3, (16, 16, 16))):   # FlowField
        out.append((ci, co) + dims)
    out += [(96, 96, 3, 8, 8), (96, 96, 5, 16, 16), (96, 96, 6, 16, 16), (96, 96, 4, 12, 12), (96, 96, 4, 20, 24), (40, 96, 4, 16, 16),
            (24, 96, 2, 8, 8), (96, 100, 4, 16, 16), (96, 64, 4, 16, 16), (1536, 96, 4, 16, 16), (1536, 1536, 2, 8, 8), (768, 768, 4, 16, 16),
            (480, 96, 4, 16, 16), (384, 96, 2, 16, 16), (192, 192, 2, 32, 32), (96, 96, 4, 8, 8), (96, 96, 2, 8, 8)]
    return out


def shapes():
    seen, out = set(), []
    for ci, co, d, h, w in layers():
        for a, b in ((ci, co), (co, ci)):   # (swapped: the bwd-data launch)
            for n in BATCHES:
                s = (n, a, b, d, h, w)
                if s not in seen:
                    seen.add(s)
                    out.append(s)
    return out


def settings():
    """name -> (environment, half-products flag): every switch of F16x3Switches at every value the code distinguishes."""
    out = {"none": ({}, 0), "half_products": ({}, 1)}
    one = {"MPHIP_F16X3_TILE": ("0",), "MPHIP_F16X3_SPLITS": ("1", "2", "3", "4", "8"), "MPHIP_F16X3_OLD_SPLITS": ("1",), "MPHIP_F16X3_NO_PERSIST": ("1",),
           "MPHIP_F16X3_XCD": ("0",), "MPHIP_WINOGRAD": ("0",), "MPHIP_WINOGRAD_D2": ("0",), "MPHIP_WINOGRAD_MIN_TILES": ("1", "192", "1000000"),
           "MPHIP_WINOGRAD_PACK": ("0",), "MPHIP_WINO_PP": ("0", "1", "2"), "MPHIP_ROI_THIRDS": ("0",), "MPHIP_CONV_CUS": ("240",),
           "MPHIP_GN_EPILOGUE": ("0",), "MPHIP_F16X3_K1_KS": ("4",), "MPHIP_F16X3_K1_MIN": ("1", "100000"), "MPHIP_F16X3_K1_NT": ("1",)}
    for name, values in one.items():
        for v in values:
            out[f"{name}={v}"] = ({name: v}, 0)
    out["MPHIP_WINO_PP=2,half_products"] = ({"MPHIP_WINO_PP": "2"}, 1)
    for v in ("0", "1", "2"):   # what the GPU tests use
        out[f"MPHIP_WINOGRAD_MIN_TILES=1,MPHIP_WINO_PP={v}"] = ({"MPHIP_WINOGRAD_MIN_TILES": "1", "MPHIP_WINO_PP": v}, 0)
    out["MPHIP_F16X3_SPLITS=2,MPHIP_WINOGRAD=0"] = ({"MPHIP_F16X3_SPLITS": "2", "MPHIP_WINOGRAD": "0"}, 0)
    return out


def rows(half_products):
    """One row per shape from the library loaded in THIS process (its environment is the setting)."""
    lib = ctypes.CDLL(LIB)
    i8 = [ctypes.c_int] * 8
    for name, res, args in (("mphip_conv3d_supported", ctypes.c_int, i8), ("mphip_conv3d_kernel_variant", ctypes.c_int, i8),
                            ("mphip_conv3d_splits", ctypes.c_int, i8), ("mphip_conv3d_workspace_bytes", ctypes.c_size_t, i8),
                            ("mphip_conv3d_gn_workspace_bytes", ctypes.c_size_t, i8 + [ctypes.c_int]),
                            ("mphip_conv3d_roi_granule", ctypes.c_int, i8 + [ctypes.c_void_p]),
                            ("mphip_conv3d_roi_workspace_bytes", ctypes.c_size_t, i8), ("mphip_packed_weight_bytes", ctypes.c_size_t, [ctypes.c_int] * 4),
                            ("mphip_debug_conv3d_plan", ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.c_void_p]),
                            ("mphip_conv3d_set_half_products", ctypes.c_int, [ctypes.c_int])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    lib.mphip_conv3d_set_half_products(half_products)
    out = []
    for n, ci, co, d, h, w in shapes():
        row = []
        for k, p in KP:
            a = (n, ci, co, d, h, w, k, p)
            tile = (ctypes.c_int * 3)(0, 0, 0)
            row += [lib.mphip_conv3d_supported(*a), lib.mphip_conv3d_kernel_variant(*a), lib.mphip_conv3d_splits(*a),
                    lib.mphip_conv3d_workspace_bytes(*a), lib.mphip_conv3d_gn_workspace_bytes(*a, GROUPS),
                    lib.mphip_conv3d_roi_granule(*a, tile), tile[0], tile[1], tile[2], lib.mphip_conv3d_roi_workspace_bytes(*a),
                    lib.mphip_packed_weight_bytes(co, ci, k, p)]
        for roi in (0, 1):
            plan = (ctypes.c_int * 12)(*([-1] * 12))
            row += [lib.mphip_debug_conv3d_plan(n, ci, co, d, h, w, roi, plan)] + list(plan)
        out.append(row)
    return out


SWITCHES = ("MPHIP_F16X3_TILE", "MPHIP_F16X3_SPLITS", "MPHIP_F16X3_OLD_SPLITS", "MPHIP_F16X3_NO_PERSIST", "MPHIP_F16X3_XCD", "MPHIP_WINOGRAD",
            "MPHIP_WINOGRAD_D2", "MPHIP_WINOGRAD_MIN_TILES", "MPHIP_WINOGRAD_PACK", "MPHIP_WINO_PP", "MPHIP_ROI_THIRDS", "MPHIP_CONV_CUS",
            "MPHIP_GN_EPILOGUE", "MPHIP_F16X3_K1_KS", "MPHIP_F16X3_K1_MIN", "MPHIP_F16X3_K1_NT", "MPHIP_CONV_GATHER", "MPHIP_GATHER_TARGET_WAVES",
            "MPHIP_GATHER_MIN_CH", "MPHIP_GATHER_MAX_SPLITS")


def run_setting(name):
    """The rows of one setting, from a fresh child process."""
    env_add, _ = settings()[name]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(env_add)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, capture_output=True, text=True, check=True)
    return json.loads(r.stdout)


def record():
    """{"columns", "groups", "settings": {name: {"env", "half_products"}}, "shapes", "rows": [setting][shape][column]}"""
    table = {"columns": COLUMNS, "groups": GROUPS, "settings": {}, "shapes": [list(s) for s in shapes()], "rows": []}
    for name, (env, half) in settings().items():
        table["settings"][name] = {"env": env, "half_products": half}
        table["rows"].append(run_setting(name))
    return table


def dump(table, path):
    """The file keeps columns and settings readable; the numbers (shapes and the full rows of every setting, mostly repeats of the "none"
    rows) travel as xz-compressed JSON in base64, which load() expands again.  `--show FILE` prints them."""
    head = {k: table[k] for k in ("columns", "groups", "settings")}
    body = json.dumps({"shapes": table["shapes"], "rows": table["rows"]}, separators=(",", ":")).encode()
    head["shapes_and_rows_json_xz_base64"] = base64.b64encode(lzma.compress(body, preset=9 | lzma.PRESET_EXTREME)).decode()
    with open(path, "w") as f:
        json.dump(head, f, indent=1)
        f.write("\n")


def load(path):
    with open(path) as f:
        table = json.load(f)
    table.update(json.loads(lzma.decompress(base64.b64decode(table.pop("shapes_and_rows_json_xz_base64")))))
    return table


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--child":
        print(json.dumps(rows(settings()[sys.argv[2]][1])))
    elif len(sys.argv) == 3 and sys.argv[1] == "--show":
        t = load(sys.argv[2])
        print("setting\tN,Ci,Co,D,H,W\t" + "\t".join(t["columns"]))
        for name, per_shape in zip(t["settings"], t["rows"]):
            for shape, row in zip(t["shapes"], per_shape):
                print(name + "\t" + ",".join(map(str, shape)) + "\t" + "\t".join(map(str, row)))
    elif len(sys.argv) == 2:
        dump(record(), sys.argv[1])
        print(f"recorded {len(shapes())} shapes x {len(settings())} settings from {LIB}")
    else:
        sys.exit(__doc__)
