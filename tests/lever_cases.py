"""What tests/test_gpu_levers.py and the host tests of the levers are built from (a helper, not a test module; no device
is needed to import it): every `M2D_*` lever of DESIGN.md section 16 in its OTHER position.

The library reads a switch once per process, so an arm runs in a fresh child process with the arm's environment:
run_arm(name, out_path) executes the arm's work items there, reads the route counters of the library before and after
(csrc/m2d_common.h: m2d_route_hit) and saves what it saw. The parent asserts from that file.

  ARMS     name -> Arm: env (the lever values), work (items, below), hit / miss (route names that must count >= 1 / 0 in
           the child), default_hit / default_miss (the same for the parent's own run of the arm's cases WITHOUT the
           environment: the opposite position, i.e. the route the suite's other tests are assumed to reach), same_bits
           (cases whose results equal the default arm's bit for bit), thin_wg (the workgroups-per-CU value the
           persistent single-channel forward must report)
  EXEMPT   lever -> why it has no arm
  CASES    the cases no other table had, in the form of tests/placement_cases.py: Case, with plain-torch fp64 references

A work item is a tuple. ("<case name>",) or ("<case name>", {"plan": (bm, splits)}): a case of placement_cases.CASES or
of CASES here, run on aligned operands against its own fp64 reference and its own bound (P.within), optionally under a
forced launch plan. ("tests.module:function", arg, ...): an existing GPU test function called as a plain function with
literal arguments (an argument "@tests.module:NAME:i" is element i of that module's list NAME); these assert for
themselves, against fp64 torch or the reference's golden files. An entry of hit / miss that is a tuple means "any of" /
"none of" its names.
"""
import ctypes
import functools
import importlib
import math
import time
import traceback

import torch
import torch.nn.functional as F

from tests import placement_cases as P
from tests.placement_cases import Case, gen, mf

DEV = "cuda:0"

# ----------------------------------------------------------------------------------------------- the route witness
_h = None


def _handle():
    global _h
    if _h is None:
        from music2dance_amd import _lib
        _h = ctypes.CDLL(_lib.LIB_PATH)
        _h.m2d_debug_route_names.restype = ctypes.c_char_p
        _h.m2d_debug_route_names.argtypes = []
        _h.m2d_debug_routes.restype = ctypes.c_int
        _h.m2d_debug_routes.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
        _h.m2d_debug_thin_wg_per_cu.restype = ctypes.c_int
        _h.m2d_debug_thin_wg_per_cu.argtypes = []
    return _h


def route_names():
    """csrc/m2d_runtime.hip: m2d_debug_route_names, in enum order"""
    return _handle().m2d_debug_route_names().decode().split(",")


def routes():
    """-> {route name: launches of that form since the library was loaded}"""
    names = route_names()
    buf = (ctypes.c_ulonglong * len(names))()
    n = _handle().m2d_debug_routes(buf, len(names))
    assert n == len(names), (n, len(names))
    return dict(zip(names, (int(v) for v in buf)))


def routes_since(before):
    return {k: v - before[k] for k, v in routes().items()}


def thin_wg_per_cu():
    """workgroups per CU the last persistent single-channel forward sized its grid with (0: none ran)"""
    return int(_handle().m2d_debug_thin_wg_per_cu())


def route_misses(seen, hit, miss):
    """-> the list of complaints of `seen` ({route: count}) against hit / miss"""
    bad = []
    for h in hit:
        names = (h,) if isinstance(h, str) else h
        if not any(seen[n] >= 1 for n in names):
            bad.append("never ran: " + " / ".join(names))
    for m in miss:
        for n in ((m,) if isinstance(m, str) else m):
            if seen[n] != 0:
                bad.append("ran %d times: %s" % (seen[n], n))
    return bad


# ------------------------------------------------------------------------------------------------------ new cases
CASES = []


def _case(*a, **kw):
    CASES.append(Case(*a, **kw))


def _conv_ops(shape, seed=0):
    B, Cin, L, Cout, ks, s, p = shape
    Lout = (L + 2 * p - ks) // s + 1
    return {"x": gen(B, Cin, L, seed=seed + 1), "w": gen(Cout, Cin, ks, seed=seed + 2, scale=1.0 / math.sqrt(Cin * ks)),
            "bias": gen(Cout, seed=seed + 3, scale=0.1), "dy": gen(B, Cout, Lout, seed=seed + 4),
            "ymask": gen(B, Cout, Lout, seed=seed + 5), "yres": gen(B, Cout, Lout, seed=seed + 6),
            "xmask": gen(B, Cin, L, seed=seed + 7), "xres": gen(B, Cin, L, seed=seed + 8),
            "y": torch.zeros(B, Cout, Lout), "dx": torch.zeros(B, Cin, L)}


def _pick(shape, names):
    return lambda: {k: v for k, v in _conv_ops(shape).items() if k in names}


def _conv_fwd(tag, shape, form):
    """the forms of placement_cases._conv_fwd, for a layer that is not in its table"""
    B, Cin, L, Cout, ks, s, p = shape
    conv = lambda t: F.conv1d(t["x"], t["w"], t["bias"], stride=s, padding=p)
    tol = P.TOL_PATH
    if form == "plain":
        names, written = ("x", "w", "bias", "y"), ("y",)
        run = lambda K, t: (K.conv1d_fwd(t["x"], t["w"], t["bias"], s, p, act=1, out=t["y"]),)
        ref = lambda t: (F.relu(conv(t)),)
    elif form == "full":
        names, written = ("x", "w", "bias", "yres", "ymask", "y"), ("y",)
        run = lambda K, t: (K.conv1d_fwd(t["x"], t["w"], t["bias"], s, p, act=2, slope=0.2, residual=t["yres"],
                                         out_mask=t["ymask"], out_mask_slope=0.2, out=t["y"]),)
        ref = lambda t: (F.leaky_relu(conv(t), 0.2) * mf(t["ymask"], 0.2) + t["yres"],)
    else:
        assert form == "stats"
        names, written, tol = ("x", "w", "bias"), (), [P.TOL_PATH, P.TOL_SUMS]
        run = lambda K, t: K.conv1d_fwd(t["x"], t["w"], t["bias"], s, p, act=2, slope=0.2, with_stats=True)

        def ref(t):
            y = F.leaky_relu(conv(t), 0.2)
            return y, torch.stack((y.sum((0, 2)), (y * y).sum((0, 2))), 1).reshape(-1)
    _case("conv1d_fwd %s %s" % (tag, form), "conv1d_fwd", _pick(shape, names), run, ref, names, written, tol=tol)


def _conv_bwd_data(tag, shape, form):
    B, Cin, L, Cout, ks, s, p = shape
    gx = lambda t: torch.nn.grad.conv1d_input((B, Cin, L), t["w"], t["dy"], stride=s, padding=p)
    if form == "plain":
        names = ("dy", "w", "dx")
        run = lambda K, t: (K.conv1d_bwd_data(t["dy"], t["w"], L, s, p, out=t["dx"]),)
        ref = lambda t: (gx(t),)
    else:
        assert form == "epi"
        names = ("dy", "w", "xmask", "xres", "dx")
        run = lambda K, t: (K.conv1d_bwd_data(t["dy"], t["w"], L, s, p, out_mask=t["xmask"], out_mask_slope=0.2,
                                              residual=t["xres"], out=t["dx"]),)
        ref = lambda t: ((gx(t) + t["xres"]) * mf(t["xmask"], 0.2),)
    _case("conv1d_bwd_data %s %s" % (tag, form), "conv1d_bwd_data", _pick(shape, names), run, ref, names, ("dx",))


def _conv_bwd_weight_masked(tag, shape):
    B, Cin, L, Cout, ks, s, p = shape
    names = ("x", "dy", "ymask")
    run = lambda K, t: K.conv1d_bwd_weight(t["x"], t["dy"], ks, s, p, dy_mask=t["ymask"], dy_mask_slope=0.2, with_bias=True)

    def ref(t):
        dy = t["dy"] * mf(t["ymask"], 0.2)
        return torch.nn.grad.conv1d_weight(t["x"], (Cout, Cin, ks), dy, stride=s, padding=p), dy.sum((0, 2))
    _case("conv1d_bwd_weight %s masked" % tag, "conv1d_bwd_weight", _pick(shape, names), run, ref, names, tol=P.TOL_PARAM)


# (B, Cin, L, Cout, ks, stride, pad): the smallest layers that reach a form only a lever opens
LAYERS = {
    "tall.128": (2, 128, 260, 64, 25, 4, 11),      # k25 / s4 backward-data at 128 input channels: phase-major under M2D_SUBPIXEL_TALL_MAXCIN=128
    "k4.128": (1, 128, 256, 64, 25, 4, 11),        # tap-vectorised forward at 128 input channels under M2D_K4_MAXCIN=128
    # statistics over K = 3200 (200 chunks). The plan model asks 50 splits here (100 at Cin = 256, 128 from 384 to 1024
    # channels; tests/test_levers_host.py pins it): beyond the 16 one launch finishes, so this launch is never split
    "stats.k3200": (4, 128, 25, 128, 25, 1, 12),
    # ... and the one that is: K = 384 (24 chunks), 6 splits in one launch - placement_cases' "unet.k3.25" with statistics
    "stats.k384": P.CONV_LAYERS["unet.k3.25"],
    "stats.n125": (5, 32, 50, 64, 4, 2, 1),        # N = 5 x 25 = 125 columns: output rows not on 16 bytes
    # the two layers of tests/test_gpu_gemm_plans.py (80 K chunks and more in every pass), here under the plans the MODEL
    # gives them: the smallest shapes at which M2D_PLAN_MODEL and M2D_SLAB_COST move a plan
    "plan.s1": (12, 40, 100, 133, 27, 1, 13),
    "plan.s2": (20, 72, 101, 133, 17, 2, 8),
}
for _f in ("plain", "epi"):
    _conv_bwd_data("tall.128", LAYERS["tall.128"], _f)
for _f in ("plain", "full"):
    _conv_fwd("k4.128", LAYERS["k4.128"], _f)
for _l in ("stats.k3200", "stats.k384", "stats.n125"):
    _conv_fwd(_l, LAYERS[_l], "stats")
_conv_bwd_weight_masked("tcn.50", P.CONV_LAYERS["tcn.50"])
_conv_fwd("plan.s1", LAYERS["plan.s1"], "plain")
_conv_bwd_data("plan.s1", LAYERS["plan.s1"], "plain")
_conv_fwd("plan.s2", LAYERS["plan.s2"], "plain")


def _forced_gemm(splits):
    """placement_cases' mode-0 GEMM (480 x 256 x 256: 16 K chunks, 4 splits at most) under the forced plan (64 rows,
    `splits`) on the stream as it is: with the stream's tickets the split finishes inside the launch (up to
    M2D_FUSE_MAX splits), without them (M2D_FUSED_SPLITK=0) in the reduction launch"""
    def run(K, t):
        if K.name != "hip":
            return (K.gemm(0, t["a"], t["b"], t["bias"], act=2, slope=0.2, out=t["c"]),)
        from tests import plan_cases
        with plan_cases.forced_plan(64, splits):
            return (K.gemm(0, t["a"], t["b"], t["bias"], act=2, slope=0.2, out=t["c"]),)
    _case("gemm mode 0 forced 64 x %d" % splits, "gemm",
          lambda: {k: v for k, v in P._gemm_ops(0).items() if k in ("a", "b", "bias", "c")}, run,
          lambda t: (F.leaky_relu(t["a"] @ t["b"].t() + t["bias"], 0.2),), ("a", "b", "bias", "c"), ("c",))


_forced_gemm(2)
_forced_gemm(3)


@functools.lru_cache(maxsize=None)
def case_table():
    t = {c.name: c for c in P.CASES}
    for c in CASES:
        assert c.name not in t, c.name
        t[c.name] = c
    return t


# ------------------------------------------------------------------------------------------------------------ arms
class Arm:
    def __init__(self, name, env, work, hit=(), miss=(), default_hit=(), default_miss=(), same_bits=(), thin_wg=None,
                 plan_moves=()):
        self.name, self.env, self.work = name, dict(env), [tuple(w) for w in work]
        self.hit, self.miss, self.default_hit, self.default_miss = tuple(hit), tuple(miss), tuple(default_hit), tuple(default_miss)
        self.same_bits, self.thin_wg, self.plan_moves = tuple(same_bits), thin_wg, tuple(plan_moves)
        assert all(k.startswith("M2D_") and isinstance(v, str) for k, v in self.env.items()), name

    def case_items(self):
        return [w for w in self.work if not is_function(w)]

    def __repr__(self):
        return self.name


def is_function(item):
    return item[0].startswith("tests.") and ":" in item[0]


ARMS = {}


def arm(name, env, work, **kw):
    assert name not in ARMS, name
    ARMS[name] = Arm(name, env, work, **kw)


def fwd(layer, *forms):
    return [("conv1d_fwd %s %s" % (layer, f),) for f in forms]


def bwdD(layer, *forms):
    return [("conv1d_bwd_data %s %s" % (layer, f),) for f in forms]


def bwdW(layer, *forms):
    return [("conv1d_bwd_weight %s %s" % (layer, f),) for f in forms]


def planned(items, bm, splits):
    return [(i[0], {"plan": (bm, splits)}) for i in items]


_DENSE = "tests.test_gpu_gemm_plans:test_dense_gemm_under_every_plan"


def dense(mode, width, epi):
    return (_DENSE, mode, width, epi)


DL = ("gemm_dl_tall", "gemm_dl8", "gemm_dl4_128", "gemm_dl_small")
TCN = ("conv_to_tcn_fwd", "conv_to_tcn_bwd_data", "conv_to_tcn_wgrad", "tcn_ns4", "tcn_ns8", "tcn_nt96", "tcn_nt64", "tcn_nt48",
       "tcn_nt32", "tcn_nt16", "tcn_wgrad")
# mode 2 = both operands row-fast and unmasked: the LDS-direct kernels' GEMM; every plan the function walks, 128 rows included
_DENSE_MODE2 = [dense(2, w, "plain") for w in ("n260", "n260-odd-pitch", "n261")] + [dense(2, w, "bias+leaky") for w in ("n260", "n261")]
_SUBPIXEL_BWD = bwdD("subpixel", "plain", "epi") + bwdD("subpixel.ragged", "plain", "epi")

# ---- csrc/gemm_engine.hip
arm("dl-off", {"M2D_DL": "0"},
    _DENSE_MODE2 + fwd("unet.k3.25", "plain") + bwdD("unet.k3.25", "plain") + bwdW("unet.k3.25", "plain") + _SUBPIXEL_BWD,
    # subpixel_tall() asks m2d_dl_enabled(): the 32-channel layer keeps the (ci, r) image the register-staging kernel can
    # read; the 64-channel one (M = 256 > M2D_SUBPIXEL_MAXROWS) is sub-pixel only in the phase-major form: polyphase
    hit=("gemm_reg_rr", "bwd_subpixel_cir", "bwd_polyphase"), miss=DL + ("bwd_subpixel_tall",),
    default_hit=("gemm_dl_tall", "bwd_subpixel_tall", ("gemm_dl8", "gemm_dl4_128", "gemm_dl_small")), default_miss=("bwd_subpixel_cir",))
# (a dense GEMM's output map never qualifies for the 16-byte epilogue outside the two-launch slabs, so by default only
# those of its launches run eight waves; the conv forward with 16-byte rows does, here forced to 128-row tiles)
arm("dl8-off", {"M2D_DL8": "0"}, _DENSE_MODE2 + planned(fwd("enc.c1", "plain", "full"), 128, 1),
    hit=("gemm_dl4_128",), miss=("gemm_dl8",), default_hit=("gemm_dl8",), default_miss=("gemm_dl4_128",))
arm("dl8-off-quad", {"M2D_DL8": "0", "M2D_SUBPIXEL_TALL": "0"}, planned(bwdD("subpixel", "plain", "epi"), 128, 1),
    hit=("bwd_subpixel_cir", "gemm_dl4_128"), miss=("gemm_dl8", "gemm_dl_tall"), default_hit=("gemm_dl_tall",))
arm("wide-off", {"M2D_WIDE_EPILOGUE": "0"},
    [dense(m, "n260", "plain") for m in (0, 1, 2)] + [dense(0, "n260", "masks"), dense(1, "n260", "masks"), dense(2, "n260", "out_mask")]
    + fwd("enc.c1", "plain", "full", "sum", "stats") + fwd("k4pair.a", "plain"),
    hit=("epi_one",), miss=("epi_wide",), default_hit=("epi_wide",))
arm("tile-map-off", {"M2D_TILE_MAP": "0"},
    [dense(m, w, "plain") for m in (0, 1, 2) for w in ("n260", "n261")] + [("gemm mode %d" % m,) for m in (0, 1, 2)]
    + fwd("enc.c1", "plain") + bwdW("unet.k3.25", "plain"),
    hit=("tile_map_off",), default_miss=("tile_map_off",),
    # m2d_tile_of is a bijection of the same tiles: a tile's sum (and a fused split-K's, read back in split order) does not
    # depend on which workgroup computes it. Not the weight gradient's bias (channel sums: fp64 atomics)
    same_bits=("gemm mode 0", "gemm mode 1", "gemm mode 2", "conv1d_fwd enc.c1 plain"))
arm("splitk-two-launch", {"M2D_FUSED_SPLITK": "0"},
    [("gemm mode 0",), ("gemm mode 2",), ("gemm mode 0 forced 64 x 3",)] + fwd("enc.c1", "stats") + fwd("stats.k384", "stats")
    + bwdW("unet.k3.25", "plain"),
    hit=("splitk_two_launch",), miss=("splitk_one_launch", "stats_split"), default_hit=("splitk_one_launch", "stats_split"))
arm("fuse-max", {"M2D_FUSE_MAX": "2"}, [("gemm mode 0 forced 64 x 3",), ("gemm mode 0 forced 64 x 2",)],
    hit=("splitk_two_launch", "splitk_one_launch"), default_hit=("splitk_one_launch",), default_miss=("splitk_two_launch",))
arm("stats-split-off", {"M2D_STATS_SPLIT": "0"}, fwd("enc.c1", "stats") + fwd("stats.k3200", "stats") + fwd("stats.k384", "stats"),
    miss=("stats_split",), default_hit=("stats_split",))
arm("stats-narrow-off", {"M2D_STATS_NARROW_FAST": "0"}, fwd("stats.n125", "stats"),
    hit=("stats_general", "epi_one"), miss=("epi_wide",), default_hit=("epi_one",), default_miss=("stats_general",))
_PLAN_WORK = [i for l in ("unet.k3.25", "enc.c1", "subpixel") for i in fwd(l, "plain") + bwdD(l, "plain") + bwdW(l, "plain")]
# These three change only which plan a launch takes: no route. Their witness is the plan itself - plan_moves names
# (layer, pass) pairs of the arm's work whose plan (plan_of, below) must differ between the child and the parent.
arm("plan-rounds-off", {"M2D_PLAN_ROUNDS": "0"}, _PLAN_WORK, plan_moves=[("unet.k3.25", "bwdW")])
arm("plan-model-5", {"M2D_PLAN_MODEL": "5"}, _PLAN_WORK + bwdD("plan.s1", "plain") + fwd("plan.s2", "plain"),
    plan_moves=[("plan.s1", "bwdD"), ("plan.s2", "fwd")])
arm("slab-cost", {"M2D_SLAB_COST": "4"}, _PLAN_WORK + fwd("plan.s1", "plain") + bwdD("plan.s1", "plain"),
    plan_moves=[("plan.s1", "fwd"), ("plan.s1", "bwdD")])

# ---- csrc/conv1d.hip
_TALL_WORK = _SUBPIXEL_BWD + bwdD("k4pair.a", "plain")
arm("tall-off", {"M2D_SUBPIXEL_TALL": "0"}, _TALL_WORK,
    hit=("bwd_subpixel_cir",), miss=("bwd_subpixel_tall", "gemm_dl_tall"),
    default_hit=("bwd_subpixel_tall", "gemm_dl_tall", "bwd_subpixel_cir"))   # (k4pair.a, 16 channels: (ci, r) in both arms)
arm("subpixel-off", {"M2D_SUBPIXEL": "0"}, _TALL_WORK,
    hit=("bwd_polyphase",), miss=("bwd_subpixel_tall", "bwd_subpixel_cir", "gemm_dl_tall"),
    default_hit=("bwd_subpixel_tall", "bwd_subpixel_cir"), default_miss=("bwd_polyphase",))
arm("subpixel-rows", {"M2D_SUBPIXEL_MAXROWS": "256", "M2D_SUBPIXEL_TALL": "0"}, bwdD("subpixel.ragged", "plain", "epi"),
    hit=("bwd_subpixel_cir",), miss=("bwd_subpixel_tall", "bwd_polyphase"), default_hit=("bwd_subpixel_tall",))
arm("tall-wide", {"M2D_SUBPIXEL_TALL_MAXCIN": "128"}, bwdD("tall.128", "plain", "epi"),
    hit=("bwd_subpixel_tall", "gemm_dl_tall"), miss=("bwd_polyphase",), default_hit=("bwd_polyphase",),
    default_miss=("bwd_subpixel_tall", "bwd_subpixel_cir"))
arm("k4-pair-off", {"M2D_K4_PAIR": "0"}, fwd("k4pair.a", "plain", "full"),
    hit=("k4_plain",), miss=("k4_paired",), default_hit=("k4_paired",), default_miss=("k4_plain",))
arm("k4-maxcin", {"M2D_K4_MAXCIN": "128"}, fwd("k4.128", "plain", "full"),
    hit=("k4_paired",), miss=("k4_plain",), default_hit=(("gemm_dl8", "gemm_dl4_128", "gemm_dl_small"),),   # (the general engine)
    default_miss=("k4_paired", "k4_plain"))
arm("k4-off", {"M2D_K4": "0"}, fwd("k4pair.a", "plain") + fwd("k4plain.a", "plain"),
    miss=("k4_paired", "k4_plain"), default_hit=("k4_paired", "k4_plain"))

# ---- csrc/tcn.hip
_TCN_WGRAD_WORK = bwdW("tcn.3", "plain", "masked") + bwdW("tcn.50", "plain", "masked")
arm("tcn-off", {"M2D_TCN": "0"},
    [i for l in ("tcn.3", "tcn.50") for i in fwd(l, "plain", "full", "sum") + bwdD(l, "plain", "epi", "full")] + _TCN_WGRAD_WORK,
    miss=TCN, default_hit=("conv_to_tcn_fwd", "conv_to_tcn_bwd_data", "conv_to_tcn_wgrad", "tcn_ns8", "tcn_wgrad", "tcn_nt16", "tcn_nt32"))
arm("tcn-wgrad-off", {"M2D_TCN_WGRAD": "0"}, _TCN_WGRAD_WORK + fwd("tcn.3", "plain"),
    hit=("conv_to_tcn_fwd", "tcn_ns8"), miss=("tcn_wgrad", "conv_to_tcn_wgrad"), default_hit=("tcn_wgrad", "conv_to_tcn_wgrad"))
_TCN_EPI = "tests.test_gpu_tcn:test_temporal_conv_epilogues"
arm("tcn-ns4", {"M2D_TCN_NS": "4"}, [(_TCN_EPI, (3, 128, 120)), (_TCN_EPI, (60, 128, 120))] + fwd("tcn.3", "plain") + bwdD("tcn.3", "plain"),
    hit=("tcn_ns4",), miss=("tcn_ns8",), default_hit=("tcn_ns8",), default_miss=("tcn_ns4",))
# 360 positions in 96-column tiles: three whole tiles and one of 72 (the model's own choice here: 16 columns)
arm("tcn-nt96", {"M2D_TCN_NT": "96"}, fwd("tcn.3", "full") + bwdD("tcn.3", "full"),
    hit=("tcn_nt96",), miss=("tcn_nt16",), default_hit=("tcn_nt16",), default_miss=("tcn_nt96",))

# ---- csrc/conv1d_thin.hip
arm("thin-long-off", {"M2D_THIN_LONG": "0"}, fwd("enc.c0", "plain") + bwdW("enc.c0", "plain") + bwdD("enc.c0", "plain"),
    miss=("thin_long", "conv_to_thin_long"), default_hit=("thin_long", "conv_to_thin_long"))
_THIN_WORK = fwd("wg.l1", "plain") + [("conv1d_fwd_windows wavegan.l1-thin",),
                                      ("tests.test_gpu_thin_persistent:test_k25_forward_over_several_tiles_per_wave",
                                       "@tests.thin_cases:K25_FWD_CASES:0")]
# y: a tile's sum does not depend on the wave that walks it (the statistics do: one partial per wave, and they are not in
# these two cases)
_THIN_BITS = ("conv1d_fwd wg.l1 plain", "conv1d_fwd_windows wavegan.l1-thin")
arm("thin-grid-1", {"M2D_THIN_WG_PER_CU": "1"}, _THIN_WORK, hit=("thin_persistent",), default_hit=("thin_persistent",),
    same_bits=_THIN_BITS, thin_wg=1)
arm("thin-grid-16", {"M2D_THIN_WG_PER_CU": "16"}, _THIN_WORK, hit=("thin_persistent",), default_hit=("thin_persistent",),
    same_bits=_THIN_BITS, thin_wg=16)

# ---- csrc/bn.hip, csrc/pointwise.hip, csrc/gru.hip
arm("bn-vec-off", {"M2D_BN_VEC_ROWS": "0"},
    [(n + " 4x128x120",) for n in ("bn_fwd training", "bn_stats", "bn_bwd", "bn_bwd_stats + bn_bwd_sums", "channel_sums")],
    hit=("bn_reduce_scalar",), miss=("bn_reduce_vec",), default_hit=("bn_reduce_vec",))
_UP = [("%s %s" % (op, s),) for s in ("2x4x200", "4x5x25", "2x3x1") for op in ("upsample2_fwd", "upsample2_bwd")]
arm("upsample-flat-off", {"M2D_UPSAMPLE_FLAT": "0"}, _UP + [("bn_fwd_sums_upsample2 5x8x50",)],
    hit=("up_fwd_vec", "up_fwd_row", "up_bwd_plain"), miss=("up_fwd_flat", "up_bwd_flat"),
    default_hit=("up_fwd_flat", "up_bwd_flat", "up_fwd_row"), default_miss=("up_fwd_vec",),
    # elementwise: every form evaluates the same two expressions per output element (the placement test holds the per-row
    # forms to the flat ones the same way)
    same_bits=tuple(i[0] for i in _UP))
arm("gru-step", {"M2D_PERSISTENT_GRU": "0"},
    [("gru_stack_%s %s persistent" % (d, t),) for t in ("h12", "h240") for d in ("fwd", "bwd")],
    hit=("gru_fwd_steps", "gru_bwd_steps"), miss=("gru_fwd_persistent", "gru_bwd_persistent"),
    default_hit=("gru_fwd_persistent", "gru_bwd_persistent"))

# ---- levers read at import time or in a constructor: the phase-3 engine's 8-step trace against the reference's golden
# trace and final parameter sums (tests/test_product_parity.py: test_p3_trace), and the attribute the lever sets
_ENGINE = "tests.lever_cases:engine_trace"
for _name, _lever, _value, _p3case in (
        ("fused-bias-off", "M2D_FUSED_BIAS", "0", ("default", "id", False)),
        ("premask-off", "M2D_PREMASK", "0", ("default", "id", False)),
        ("separate-bias-off", "M2D_SEPARATE_BIAS", "0", ("default", "id", False)),
        ("engine-k4-off", "M2D_K4", "0", ("default", "id", False)),
        ("adam-torch", "M2D_ADAM", "torch", ("default", "id", False)),
        ("keep-packs-off", "M2D_KEEP_PACKS", "0", ("default", "id", False)),
        ("branch-overlap-off", "M2D_BRANCH_OVERLAP", "0", ("default", "id", False)),
        ("early-pair-off", "M2D_EARLY_PAIR", "0", ("default", "id", False)),
        ("merge-audio-bwd-off", "M2D_MERGE_AUDIO_BWD", "0", ("default", "id", False)),
        ("fused-bn-stats-off", "M2D_FUSED_BN_STATS", "0", ("default", "id", False)),
        ("fused-bn-then-off", "M2D_FUSED_BN_THEN", "0", ("unet", "id", True))):
    arm(_name, {_lever: _value}, [(_ENGINE, _lever, _p3case)],
        miss=("k4_paired", "k4_plain") if _lever == "M2D_K4" else ())

EXEMPT = {
    "M2D_MANUAL_CRITIC": "both positions: tests/test_gpu_p2_gan.py and tests/test_gpu_p2_cond.py (autograd against the manual schedule)",
    "M2D_REUSE_AUDIO_PATH": "both positions: tests/test_audio_path_reuse.py",
    "M2D_GRU_SMALL": "both positions: tests/test_gpu_gru_small.py (the gru_stack fallback)",
    "M2D_GRU_BWD_PERSIST": "both positions: tests/test_gpu_gru_edges.py",
    "M2D_BN_FIN_IN_APPLY": "tests/test_gpu_kernels.py::test_from_sums_forwards_with_the_separate_finalize_launch, bit-equal in a child",
    "M2D_PLAN": "read by -DM2D_TUNING builds only; superseded by m2d_debug_force_plan (tests/test_gpu_gemm_plans.py)",
    "M2D_GEN_PIPELINE": "acts only when train_step is handed inputs_ready (bench.py's loader); no parity trace drives it so",
}


# ---------------------------------------------------------------------------------------------------- running items
def resolve(item):
    """-> the Case, or the callable and its arguments, an item names (raises where it names nothing)"""
    if not is_function(item):
        assert len(item) <= 2 and (len(item) == 1 or set(item[1]) <= {"plan"}), item
        return case_table()[item[0]]
    mod, fn = item[0].split(":")
    f = getattr(importlib.import_module(mod), fn)
    args = []
    for a in item[1:]:
        if isinstance(a, str) and a.startswith("@"):
            m, name, i = a[1:].split(":")
            a = getattr(importlib.import_module(m), name)[int(i)]
        args.append(a)
    return f, args


def item_key(item):
    return item[0] if len(item) == 1 else "%s %r" % (item[0], item[1:])


def run_case(case, K, dev, plan=None, figures=None):
    """`case` on aligned operands on `dev` -> its results as CPU tensors; every figure against the case's fp64 reference
    is noted in `figures` (name -> [(figure, bound as text, within)]) BEFORE the bounds are asserted"""
    import contextlib
    from tests import plan_cases
    t = {k: v.clone().to(dev) for k, v in case.operands().items()}
    with (plan_cases.forced_plan(*plan) if plan else contextlib.nullcontext()):
        outs = tuple(case.run(K, t))
    if dev != "cpu":
        torch.cuda.synchronize()
        K.check_async_errors()
    ref = case.reference()
    assert len(outs) == len(ref), case.name
    rows = []
    for o, r, tol in zip(outs, ref, case.tols(len(ref))):
        if r is None:
            continue
        ok, fig = P.within(o, r, tol)
        rows.append((float(fig), repr(tol) if not callable(tol) else tol.__name__, bool(ok)))
    if figures is not None:
        figures[case.name] = rows
    if case.extra is not None:
        case.extra(outs, t)
    assert all(ok for _, _, ok in rows), (case.name, rows)
    return [o.detach().cpu() for o in outs]


def run_items(items, results, figures):
    """the work items in order on the HIP device; stops at the first exception (raised on)"""
    from music2dance_amd import kernels
    for item in items:
        what = resolve(item)
        if isinstance(what, Case):
            plan = item[1].get("plan") if len(item) > 1 else None
            results[item_key(item)] = run_case(what, kernels.impl(), DEV, plan, figures)
        else:
            f, args = what
            f(*args)
            torch.cuda.synchronize()


def plan_of(layer, kind):
    """-> (rc, bm, splits, fused): the plan this process's library selects for pass `kind` ("fwd", "bwdD", "bwdW") of a
    packed conv layer, asked as csrc/conv1d.hip asks (tests/test_gpu_gemm_plans.py: _query) with the workspace the
    library's own size query gives and a stream's tickets. Host arithmetic only."""
    from tests import plan_cases as C
    from tests.test_gpu_gemm_plans import _query
    conv = dict(P.CONV_LAYERS, **LAYERS)[layer]
    M, N, nchunks, phases, allow_split, penalty, plan_kind, bwd_data = _query(conv, kind)
    ws = C.launcher_ws_bytes(kind, conv, M, N)
    return C.select_plan(C.GENERAL, M, N, nchunks, phases, allow_split, penalty, plan_kind, bwd_data, 0, ws, True, C.TICKET_BYTES)


def run_arm(name, out_path):
    """In the child: the arm's work, the routes it took. Saves {results, figures, routes, thin_wg, plans, seconds, error}."""
    arm_ = ARMS[name]
    results, figures, error = {}, {}, None
    t0 = time.time()
    before = routes()
    try:
        run_items(arm_.work, results, figures)
    except Exception:   # (an M2dError, an assertion of a work item: recorded, the parent names it)
        error = traceback.format_exc()
    torch.save({"results": results, "figures": figures, "routes": routes_since(before), "thin_wg": thin_wg_per_cu(),
                "plans": {"%s %s" % m: plan_of(*m) for m in arm_.plan_moves},
                "seconds": time.time() - t0, "error": error}, out_path)


# ------------------------------------------------------------------------------------------------- the engine arms
def _engine_attr(lever, eng):
    """what the lever's position left behind in the package: -> (value seen, value of the other position)"""
    from music2dance_amd import kernels, ops
    from music2dance_amd.phase3.archis import default as arch
    if lever == "M2D_ADAM":
        return type(eng.optim_critic) is torch.optim.Adam and type(eng.optim_gen) is torch.optim.Adam, True
    seen = {"M2D_FUSED_BIAS": lambda: ops._FUSED_BIAS, "M2D_PREMASK": lambda: ops._PREMASK,
            "M2D_SEPARATE_BIAS": lambda: kernels.HipKernels._SEPARATE_BIAS, "M2D_K4": lambda: kernels.HipKernels._K4,
            "M2D_KEEP_PACKS": lambda: eng._keep_packs, "M2D_BRANCH_OVERLAP": lambda: arch.SequenceDiscriminator.overlap_branches,
            "M2D_EARLY_PAIR": lambda: eng.early_pair_pass, "M2D_MERGE_AUDIO_BWD": lambda: eng.manual_critic.merge_audio_chains,
            "M2D_FUSED_BN_STATS": lambda: arch._FUSED_BN_STATS, "M2D_FUSED_BN_THEN": lambda: arch._FUSED_BN_THEN}[lever]()
    return bool(seen), False


def engine_trace(lever, p3case):
    """tests/test_product_parity.py: test_p3_trace on the HIP device, on an engine class that remembers its instances: the
    trace and the final parameter sums against the reference's golden files (independent of every arm), then the attribute
    `lever` sets."""
    from tests import test_product_parity as T
    made = []

    class Remembered(T.Phase3Engine):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            made.append(self)
    stock = T.Phase3Engine
    T.Phase3Engine = Remembered
    try:
        T.test_p3_trace(torch.device(DEV), tuple(p3case))
    finally:
        T.Phase3Engine = stock
    assert len(made) == 1
    seen, want = _engine_attr(lever, made[0])
    assert seen == want, "%s did not reach the package: %r" % (lever, seen)
