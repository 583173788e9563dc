"""The host-side GEMV launch plan (csrc/gemv_plan.h) through the `gemv_plan` binding: no GPU.

Golden table: tests/data/gemv_plan_golden.json is the kernel trace of tools/gemv_launch_trace.py at
the commit before the plan existed (kernel name, grid, workgroup size per launch); the plan must
name the same kernel instantiation, workgroup size and -- where it did not ask the occupancy query
-- grid.  The trace's LDS column holds only a kernel's static LDS (0 or 512 B for every launch), so
the dynamic LDS bytes of every golden case are checked against `parent_lds_bytes`, a plain-Python
transcription of the byte formulas the launchers held at that commit (lg_lds_bytes, lb_lds_bytes,
cu_lds_bytes, q8_lds_bytes, launch_gemv_persistent, launch_gemv_t and LgLayout's ring), applied to
the instantiation the parent's trace names; the edge cases below add values worked out by hand.
"""
import json
import os
import re

import pytest

from aios_amd.runtime import native

E = native.load(build_if_missing=False)  # (a missing engine or binding fails the module)

GOLDEN = json.load(open(os.path.join(os.path.dirname(__file__), "data", "gemv_plan_golden.json")))
TP_RESID = 4


def QT(name):
    return getattr(E, "QT_" + name)


def plan(fmts, rows, K, B, **kw):
    return E.gemv_plan([QT(f) for f in fmts], list(rows), K, B, **kw)


def case_plan(c, **kw):
    args = dict(epi=c["epi"], act_q8=c["act_q8"], force_v1=c["force_v1"], kernel_sel=c["kernel_sel"],
                tune_grid=c["tune_grid"], x16=bool(c["x16"]), y16=bool(c["y16"]), cus=GOLDEN["cus"])
    args.update(kw)
    return plan([f for f, _ in c["segs"]], [r for _, r in c["segs"]], c["K"], c["B"], **args)


def kernel_of(p, qt0, qt1):
    """the instantiation a plan names, as the trace prints it"""
    f = p["family"]
    if f == "lds":
        return f"gemv_lds_b1<{qt0}, {qt1}, {p['B']}, {p['RSUB']}>"
    if f == "lds16":
        return f"gemv_lds16<{p['B']}, {p['R']}, {p['GPW']}>"
    if f == "cu":
        return f"gemv_cu_b1<{qt0}, {qt1}, {p['D']}>"
    if f == "q8":
        return f"gemv_q8_rows<{qt0}, {qt1}, {p['B']}, {p['U']}, {p['PIPE']}>"
    if f == "persistent":
        return f"gemv_persistent<{qt0}, {qt1}, {p['B']}, {p['U']}>"
    assert f == "v1"
    return f"gemv_kernel<{qt0}, {qt1}, {p['B']}, {p['U']}>"


# ---- the parent's LDS byte formulas, transcribed (formats by name)
W_RUNS = {"Q4_K": (32, 2), "Q5_K": (32, 2), "Q6_K": (32, 2), "Q4_0": (32, 2), "Q8_0": (16, 1), "F16": (8, 1), "BF16": (8, 1)}
BLOCK = {"Q4_K": 256, "Q5_K": 256, "Q6_K": 256, "Q4_0": 32, "Q8_0": 32, "F16": 8, "BF16": 8}
# LgPlanes: (bytes per 64-chunk group, DMA width) per weight plane
PLANES = {"Q4_K": [(1024, 16), (128, 16)], "Q5_K": [(1024, 16), (128, 16), (256, 16)],
          "Q6_K": [(1024, 16), (512, 16), (128, 16), (16, 4)], "Q4_0": [(1024, 16), (128, 16)],
          "Q8_0": [(1024, 16), (64, 16)]}


def lg_ring_bytes(fmt, rsub):
    """LgLayout<QT, RSUB>::R * slot_bytes"""
    ngs = 14 * (1 if fmt in ("Q6_K", "Q5_K") else 2)
    slot = sum(-(-ngs * bpg // (64 * dsz)) * 64 * dsz for bpg, dsz in PLANES[fmt])
    depth = 4 if slot > 28 * 1024 else (6 if slot <= 20 * 1024 else 5)
    return (depth - rsub) * slot


def parent_lds_bytes(c, cus):
    """dynamic LDS of the launch the parent's trace records for case c, and its kt_max (or None)"""
    fmts, rows, K = [f for f, _ in c["segs"]], [r for _, r in c["segs"]], c["K"]
    name, targs = c["kernel"].split("<")[0], [int(v) for v in c["kernel"].split("<")[1].rstrip(">").split(",")]
    W, R = W_RUNS[fmts[0]]
    nch, npairs = K // W, sum(rows) // 2
    grid = c["tune_grid"] if c["tune_grid"] > 0 else cus
    rup256 = lambda n: (n + 255) // 256 * 256  # noqa: E731
    if name == "gemv_lds_b1":
        B, rsub = targs[2:]
        racc = E.gemv_desc_build([QT(f) for f in fmts], rows, K, grid, 3)["racc_n"]
        head = (64 + B * racc) * 4 + B * nch * R * 8 + B * K
        return rup256(head) + max(lg_ring_bytes(fmts[0], rsub), lg_ring_bytes(fmts[-1], rsub)), None
    if name == "gemv_lds16":
        B, ring, gpw = (targs + [2])[:3]
        G = min(grid, npairs)
        racc = (2 * -(-npairs // G) + 3) & ~3
        return rup256((64 + B * racc) * 4 + B * K * 2) + ring * 14 * gpw * 1024, None
    if name == "gemv_cu_b1":
        racc = E.gemv_desc_build([QT(f) for f in fmts], rows, K, grid, 2)["racc_n"]
        return max((64 + racc) * 4 + nch * R * 8 + K + 16, 81 * 1024), None
    B = targs[2]
    if name == "gemv_q8_rows":
        return 64 * 4 + B * nch * R * 8 + B * K + 2048 + 16, K
    if name == "gemv_persistent":  # (every compiled pair shares one x layout)
        return (64 + B * K + B * K // 16 + 4) * 4, K
    assert name == "gemv_kernel"
    kt = (16384 // B) // 256 * 256
    kt = max(K if kt >= K else kt, max(8, *(BLOCK[f] for f in fmts)))
    return (64 + B * kt + B * kt // 16 + 4) * 4, kt


def test_golden_lds_bytes_are_the_parents_formulas():
    for c in GOLDEN["cases"]:
        p = case_plan(c)
        lds, kt = parent_lds_bytes(c, GOLDEN["cus"])
        assert p["lds"] == lds, c
        assert kt is None or p["kt_max"] == kt, c
        assert lds <= 160 * 1024, c


def test_golden_table_is_the_parent_trace():
    cases = GOLDEN["cases"]
    assert len(cases) >= 600 and all(c["launched"] for c in cases)
    seen = set()
    for c in cases:
        p = case_plan(c)
        qt0, qt1 = QT(c["segs"][0][0]), QT(c["segs"][-1][0])
        got = kernel_of(p, qt0, qt1)
        want = c["kernel"]
        if want.startswith("gemv_lds16<") and want.count(",") == 1:  # (a defaulted GPW is not printed)
            want = want[:-1] + ", 2>"
        assert got == want, c
        assert p["threads"] == c["wg_x"], c
        if not p["occ_grid"]:
            assert p["grid"] * p["threads"] == c["grid_x"], c
            assert p["occupancy_asked"] == 0, c
        seen.add(re.match(r"\w+", got).group(0))
    assert seen == {"gemv_lds_b1", "gemv_lds16", "gemv_cu_b1", "gemv_q8_rows", "gemv_persistent", "gemv_kernel"}


def test_occupancy_is_asked_only_by_the_unbalanced_q8_grid_and_the_persistent_kernel():
    for c in GOLDEN["cases"]:
        p = case_plan(c)
        assert p["occ_grid"] == (p["occupancy_asked"] == 1), c
        if p["occ_grid"]:
            assert p["family"] in ("q8", "persistent"), c
            # the recorded grid is the plan's at one of the occupancies the device can report
            assert any(case_plan(c, occupancy=o)["grid"] * p["threads"] == c["grid_x"] for o in range(1, 9)), c


def test_engine_questions_agree_with_the_plan():
    """gemv_engine_fits asks about the int8-activation launch of the shape (the engine's path choice
    at B >= 2 is per shape); gemv_bf16_engine_fits about the launch itself."""
    for c in GOLDEN["cases"]:
        p = case_plan(c)
        is16 = c["segs"][0][0] in ("F16", "BF16")
        q = p if (c["act_q8"] and not c["force_v1"]) else case_plan(c, act_q8=1, force_v1=0, x16=False, y16=False)
        assert p["engine_fits"] == (is16 or q["family"] == "lds"), c
        assert p["bf16_engine_fits"] == (p["family"] == "lds16"), c


# ------------------------------------------------------------------------------ edges of each rule
def test_lds_engine_needs_whole_64_chunk_groups():
    assert plan(["Q4_K"], [64], 2048, 2, cus=2)["family"] == "lds"  # K / 32 = 64 chunks per row
    assert plan(["Q4_K"], [64], 2304, 2, cus=2)["family"] == "q8"   # 72


def test_lds_engine_size_floor_is_batch_1_only():
    # Q4_K, K = 2048: 1152 B per row, two CUs: 40 KB per CU lies between 70 and 72 rows
    assert plan(["Q4_K"], [72], 2048, 1, cus=2)["family"] == "lds"
    assert plan(["Q4_K"], [70], 2048, 1, cus=2)["family"] == "q8"
    assert plan(["Q4_K"], [70], 2048, 2, cus=2)["family"] == "lds"
    assert plan(["Q4_K"], [70], 2048, 1, cus=2, kernel_sel=3)["family"] == "lds"


def test_lds_engine_160k_cap_picks_the_shallower_ring():
    # head = (64 + B * racc_n) * 4 + B * K * 1.5, rounded to 256; ring = (4 - RSUB) x 32 KB (Q4_K)
    a = plan(["Q4_K"], [16], 10240, 4, cus=2)
    b = plan(["Q4_K"], [16], 12288, 4, cus=2)
    assert (a["family"], a["RSUB"], a["lds"]) == ("lds", 1, 61952 + 3 * 32768)
    assert (b["family"], b["RSUB"], b["lds"]) == ("lds", 2, 74240 + 2 * 32768)
    assert plan(["Q4_K"], [16], 14336, 3, cus=2)["RSUB"] == 1
    c = plan(["Q4_K"], [16], 16384, 3, cus=2)
    assert (c["family"], c["B"], c["RSUB"], c["lds"]) == ("lds", 3, 2, 74240 + 2 * 32768)
    assert plan(["Q4_K"], [16], 22528, 2, cus=2)["family"] == "q8"  # B = 2 has no RSUB 2 instantiation


def test_lds_engine_batch_1_ring_depth_per_format():
    for f, rsub in (("Q4_K", 1), ("Q5_K", 1), ("Q4_0", 1), ("Q8_0", 1), ("Q6_K", 2)):
        p = plan([f], [16], 2048, 1, cus=2, kernel_sel=3)
        assert (p["family"], p["RSUB"]) == ("lds", rsub), f
    # Q6_K: 5 slots of 23808 B less RSUB; head (64 + 8) * 4 + 2048 * 1.5 = 3360 -> 3584
    assert plan(["Q6_K"], [16], 2048, 1, cus=2, kernel_sel=3)["lds"] == 3584 + 3 * 23808


def test_mixed_qkv_and_unlike_layouts():
    p = plan(["Q4_K", "Q4_K", "Q6_K"], [64, 32, 32], 2048, 2, cus=4)
    assert p["family"] == "lds" and p["np0"] == 48 and 1 <= p["g0"] < 4
    with pytest.raises(RuntimeError, match="unsupported format pair"):
        plan(["Q4_0", "Q8_0"], [16, 16], 2048, 1)
    # no kernel shares one staged x between unlike layouts: the fp32 kernel stages both
    q = plan(["Q4_0", "Q8_0"], [16, 16], 2048, 1, check=False)
    assert (q["family"], q["lds"]) == ("persistent", (64 + 2 * (2048 + 128) + 4) * 4)
    assert plan(["Q4_0"], [32], 2048, 1, act_q8=0)["lds"] == (64 + 2048 + 128 + 4) * 4


def test_q8_balanced_launch():
    def q8(rows, K, **kw):
        p = plan(["Q4_K"] if isinstance(rows, int) else ["Q4_K", "Q6_K"], [rows] if isinstance(rows, int) else rows, K, 1,
                 kernel_sel=1, cus=kw.pop("cus", 4), **kw)
        assert p["family"] == "q8"
        return p

    p = q8(40, 2048)  # 20 pairs on 4 CUs: 5 waves each; one pair per wave -> the single-buffered U = 1
    assert (p["U"], p["PIPE"], p["threads"], p["grid"], p["occ_grid"]) == (1, 1, 320, 4, False)
    assert (q8(40, 4096)["U"], q8(40, 4096)["PIPE"]) == (2, 1)   # 128 chunks per row
    assert (q8(40, 4352)["U"], q8(40, 4352)["PIPE"]) == (3, 1)   # 136: past nch <= 128
    p = q8(128, 2048)  # 64 pairs = 16 x CUs: still one pair per wave, 16 waves
    assert (p["U"], p["PIPE"], p["threads"], p["grid"]) == (1, 1, 1024, 4)
    p = q8(132, 2048, occupancy=1)  # 66 pairs: past it, the double-buffered 8-wave grid
    assert (p["U"], p["PIPE"], p["threads"], p["grid"], p["occ_grid"]) == (1, 2, 512, 4, True)
    assert q8(132, 2048, occupancy=3)["grid"] == 8  # (at most 2 per CU)
    # mixed: whole waves per format, 4 + 4 pairs on 3 CUs -> 2 + 2 waves (one format: 3 waves, 3 workgroups)
    p = q8([8, 8], 2048, cus=3)
    assert (p["threads"], p["grid"]) == (256, 2)
    assert (q8(16, 2048, cus=3)["threads"], q8(16, 2048, cus=3)["grid"]) == (192, 3)
    # tune_u: the codes, and the launcher's choice for anything else
    assert (q8(40, 2048, tune_u=13)["U"], q8(40, 2048, tune_u=13)["PIPE"]) == (3, 2)
    assert (q8(40, 2048, tune_u=5)["U"], q8(40, 2048, tune_u=5)["PIPE"]) == (5, 1)
    assert (q8(40, 2048, tune_u=9)["U"], q8(40, 2048, tune_u=9)["PIPE"]) == (1, 1)
    assert q8(40, 2048)["lds"] == 256 + 64 * 2 * 8 + 2048 + 2048 + 16 and q8(40, 2048)["kt_max"] == 2048


def test_tp_fused_stage_capacity():
    kw = dict(epi=TP_RESID, kernel_sel=1, cus=256)
    # 2048 pairs, 8 waves: one workgroup would stage 4096 values, four stage 1024 each (the cap)
    assert plan(["Q4_K"], [4096], 2048, 1, grid_cap=1, tp_fused=True, **kw)["family"] == "none"
    p = plan(["Q4_K"], [4096], 2048, 1, grid_cap=4, tp_fused=True, **kw)
    assert (p["family"], p["grid"], p["threads"]) == ("q8", 4, 512)
    with pytest.raises(RuntimeError, match="EPI_TP_RESID launch not taken by the row-pair kernel"):
        plan(["Q4_K"], [4096], 2048, 1, grid_cap=1, **kw)
    assert plan(["BF16"], [4096], 2048, 1, grid_cap=4, tp_fused=True, **kw)["family"] == "none"


def test_fp32_kernels():
    p = plan(["Q4_K"], [4096], 4096, 1, force_v1=1)
    assert (p["family"], p["U"], p["kt_max"], p["grid"], p["threads"]) == ("v1", 2, 4096, 512, 256)
    assert plan(["Q4_K"], [4096], 8192, 1, force_v1=1)["U"] == 4
    p = plan(["Q4_K"], [4096], 4096, 8, force_v1=1)
    assert (p["B"], p["U"], p["kt_max"], p["lds"]) == (8, 1, 2048, (64 + 8 * 2048 + 8 * 128 + 4) * 4)
    # the persistent kernel holds all of x: (64 + K + K / 16 + 4) * 4 <= 96 KB
    assert plan(["Q4_K"], [64], 22528, 1, act_q8=0)["family"] == "persistent"
    assert plan(["Q4_K"], [64], 23296, 1, act_q8=0)["family"] == "v1"
    assert plan(["Q4_K"], [64], 2048, 8, act_q8=0)["family"] == "v1"
    with pytest.raises(RuntimeError, match="int8-activation kernels only"):
        plan(["Q4_K"], [64], 2048, 1, act_q8=0, x16=True)


def test_checks_raise_as_launch_gemv():
    for kw, msg in ((dict(B=9), "batch must be 1..8"), (dict(rows=[12, 12]), "multiple of 8 rows"),
                    (dict(rows=[15]), "N must be even"), (dict(K=2056), "K must be a multiple of 16")):
        with pytest.raises(RuntimeError, match=msg):
            rows = kw.get("rows", [16])
            plan(["Q4_K"] * len(rows), rows, kw.get("K", 2048), kw.get("B", 1))
    for check in (True, False):
        with pytest.raises(RuntimeError, match="bad segment count"):
            plan(["Q4_K"] * 4, [8] * 4, 2048, 1, check=check)
        with pytest.raises(RuntimeError, match="bad segment count"):
            plan([], [], 2048, 1, check=check)
    with pytest.raises(RuntimeError, match="only the last segment may differ"):
        plan(["Q4_K", "Q6_K", "Q6_K"], [8, 8, 8], 2048, 1)


# ----------------------------------------------------------------------------------------- knobs
def test_knobs():
    small = dict(cus=2)
    assert plan(["Q4_K"], [64], 2048, 2, knobs={"lds": 0}, **small)["family"] == "q8"
    assert plan(["Q4_K"], [16], 2048, 1, knobs={"lds": 2}, **small)["family"] == "lds"
    assert plan(["Q4_K"], [64], 2048, 3, knobs={"lds_maxb": 2}, **small)["family"] == "q8"
    assert plan(["Q4_K"], [64], 2048, 3, knobs={"lds_maxb": 2}, kernel_sel=3, **small)["family"] == "lds"
    assert plan(["Q4_K"], [70], 2048, 1, knobs={"lds_min_kb": 39.0}, **small)["family"] == "lds"
    assert plan(["Q4_K"], [72], 2048, 1, knobs={"lds_min_kb": 41.0}, **small)["family"] == "q8"
    assert plan(["Q4_K"], [72], 2048, 1, knobs={"lds_b1_rsub": 2}, **small)["RSUB"] == 2
    assert plan(["Q4_K"], [72], 2048, 1, knobs={"lds_b1_rsub": 0}, **small)["RSUB"] == 0
    assert plan(["Q6_K"], [72], 2048, 1, knobs={"lds_b1_rsub_q6": 1}, **small)["RSUB"] == 1
    assert plan(["Q6_K"], [72], 2048, 1, knobs={"lds_b1_rsub_q6": -1, "lds_b1_rsub": 0}, **small)["RSUB"] == 0
    p = plan(["Q4_K"], [16], 2048, 1, knobs={"cu": 4}, **small)
    assert (p["family"], p["D"], p["threads"], p["lds"]) == ("cu", 4, 1024, 81 * 1024)
    assert plan(["Q4_K"], [16], 2048, 1, knobs={"cu": 8}, **small)["D"] == 8
    assert plan(["Q4_K"], [16], 2048, 1, kernel_sel=2, **small)["D"] == 8
    p = plan(["Q4_K"], [40], 2048, 1, knobs={"q8_balance": 0}, cus=4)
    assert (p["family"], p["U"], p["PIPE"], p["threads"], p["occ_grid"]) == ("q8", 1, 2, 512, True)
    bf = plan(["BF16"], [16], 2048, 1, **small)
    assert (bf["family"], bf["R"], bf["GPW"], bf["lds"]) == ("lds16", 3, 2, 4608 + 3 * 28672)
    assert plan(["BF16"], [16], 2048, 1, knobs={"bf16_lds": 0}, **small)["family"] == "persistent"
    for cfg, r, gpw in ((24, 4, 2), (14, 4, 1), (16, 6, 1)):
        p = plan(["BF16"], [16], 2048, 1, knobs={"lb_cfg": cfg}, **small)
        assert (p["R"], p["GPW"], p["lds"]) == (r, gpw, 4608 + r * gpw * 14336), cfg
        assert plan(["BF16"], [16], 2048, 2, knobs={"lb_cfg": cfg}, **small)["R"] == 3  # batch 1 only
    with pytest.raises(RuntimeError, match="unknown knob"):
        plan(["Q4_K"], [16], 2048, 1, knobs={"nope": 1})


def test_the_process_environment_does_not_reach_the_binding(monkeypatch):
    monkeypatch.setenv("AIOS_GEMV_LDS", "0")
    assert plan(["Q4_K"], [64], 2048, 2, cus=2)["family"] == "lds"
