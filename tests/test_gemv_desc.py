"""Host-built GEMV launch descriptors (csrc/gemv_desc.h) against the closed-form split the kernels
used to compute in every wave: pb = g * np // G, the mixed-format g0 / np0 rule, racc_n, and the
engine's per-slot fast / seam flags re-derived in plain Python.  No GPU needed."""
import pytest

from aios_amd.gguf.quants import GGMLType
from aios_amd.runtime import native

Q4, Q6 = int(GGMLType.Q4_K), int(GGMLType.Q6_K)
BYTES_PER_256 = {Q4: 144, Q6: 210}
SLOT_GROUPS = {Q4: 28, Q6: 14}
INF = 1 << 62


@pytest.fixture(scope="module")
def E():
    return native.load(build_if_missing=False)


def rup(n, g):
    return (n + g - 1) // g


def expected(qtypes, rows, K, grid):
    """the split as kernels/gemv_lds.h and gemv_cu.h computed it in-kernel, or None"""
    N = sum(rows)
    npairs = N // 2
    G = min(grid, npairs)
    if G < 1:
        return None
    qt0, qt1 = qtypes[0], qtypes[-1]
    mixed = qt0 != qt1
    g0, np0, racc = G, npairs, (2 * rup(npairs, G) + 3) & ~3
    if mixed:
        np0 = (N - rows[-1]) // 2
        if G < 2 or np0 < 1 or np0 >= npairs:
            return None
        b0, b1 = np0 * BYTES_PER_256[qt0], (npairs - np0) * BYTES_PER_256[qt1]
        g0 = max(1, min(G - 1, int(G * b0 / (b0 + b1) + 0.5)))
        racc = (2 * max(rup(np0, g0), rup(npairs - np0, G - g0)) + 3) & ~3
    nit = (K // 32 + 63) // 64
    seg0 = [sum(rows[:i]) for i in range(len(rows))]
    G1 = seg0[1] * nit if len(rows) > 1 else INF
    G2 = seg0[2] * nit if len(rows) > 2 else INF
    wgs = []
    for g in range(G):
        fmt1 = mixed and g >= g0
        if not fmt1:
            n, Gd = (np0, g0) if mixed else (npairs, G)
            pb, pe = g * n // Gd, (g + 1) * n // Gd
        else:
            n, Gd, gg = npairs - np0, G - g0, g - g0
            pb, pe = np0 + gg * n // Gd, np0 + (gg + 1) * n // Gd
        w = dict(fmt1=int(fmt1), r0=0, nrows=0, ngroups=0, T=0, pro=[])
        if pb < pe:
            ngs = SLOT_GROUPS[qt1 if fmt1 else qt0]
            w.update(r0=2 * pb, nrows=2 * (pe - pb), ngroups=2 * (pe - pb) * nit)
            w["T"] = rup(w["ngroups"], ngs)
            first, last = w["r0"] * nit, w["r0"] * nit + w["ngroups"] - 1
            for s in range(min(w["T"], 8)):
                a, b = first + s * ngs, first + s * ngs + ngs - 1
                seg = 2 if a >= G2 else (1 if a >= G1 else 0)
                start, nxt = (0, G1, G2)[seg], (G1, G2, INF)[seg]
                fast = b <= last and b < nxt
                w["pro"].append(dict(off=a - start, seg=seg, fast=fast, seam=b <= last and not fast))
        wgs.append(w)
    return dict(G=G, g0=g0, np0=np0, racc_n=racc, wgs=wgs)


def check(E, qtypes, rows, K, grid, variant=3):
    got = E.gemv_desc_build(qtypes, rows, K, grid, variant)
    exp = expected(qtypes, rows, K, grid)
    if exp is None:
        assert got is None
        return None
    for k in ("G", "g0", "np0", "racc_n"):
        assert got[k] == exp[k], k
    assert len(got["wgs"]) == exp["G"]
    covered = 0
    for g, (a, b) in enumerate(zip(got["wgs"], exp["wgs"])):
        for k in ("r0", "nrows", "ngroups", "T", "fmt1"):
            assert a[k] == b[k], (g, k, a[k], b[k])
        assert a["pro"][:len(b["pro"])] == b["pro"], g
        lead = 0
        for p in b["pro"]:
            if not p["fast"]:
                break
            lead += 1
        assert a["nfast"] == lead, g
        # every row exactly once, in order; the accumulators hold the largest share
        if a["nrows"]:
            assert a["r0"] == covered
            covered += a["nrows"]
            assert a["nrows"] <= got["racc_n"]
    assert covered == sum(rows)
    return got


MISTRAL = [
    ("qkv_q4", [Q4, Q4, Q4], [4096, 1024, 1024], 4096),
    ("qkv_mixed", [Q4, Q4, Q6], [4096, 1024, 1024], 4096),
    ("o", [Q4], [4096], 4096),
    ("gate_up", [Q4], [28672], 4096),
    ("down_q4k", [Q4], [4096], 14336),
    ("down_q6k", [Q6], [4096], 14336),
    ("lm_head", [Q6], [32000], 4096),
]


@pytest.mark.parametrize("name,qtypes,rows,K", MISTRAL, ids=[m[0] for m in MISTRAL])
@pytest.mark.parametrize("variant", [2, 3])
def test_mistral_shapes(E, name, qtypes, rows, K, variant):
    got = check(E, qtypes, rows, K, 256, variant)
    assert got is not None and got["G"] == 256
    assert all(w["nrows"] > 0 for w in got["wgs"])


@pytest.mark.parametrize("grid", [1, 3, 37, 256])
@pytest.mark.parametrize("qt", [Q4, Q6])
@pytest.mark.parametrize("K", [2304, 4096])
def test_ragged(E, qt, K, grid):
    check(E, [qt], [1030], K, grid)


@pytest.mark.parametrize("grid", [1, 2, 5, 37, 256, 4096])
def test_mixed_segments(E, grid):
    # d = 2048, 8 / 2 heads of 64, V in Q6_K: 384 pairs; grid 4096 > pairs is clamped to the pair count,
    # grid 1 cannot serve two formats
    got = check(E, [Q4, Q4, Q6], [512, 128, 128], 2048, grid)
    if grid == 1:
        assert got is None
    else:
        assert any(w["fmt1"] for w in got["wgs"]) and not got["wgs"][0]["fmt1"]


def test_empty_workgroups(E):
    # 4 Q4_K pairs + 16 Q6_K pairs on 20 workgroups: the byte-proportional split gives Q6_K 17
    # workgroups for its 16 pairs, so one of them owns nothing
    got = check(E, [Q4, Q6], [8, 32], 2048, 20)
    assert (got["G"], got["g0"], got["np0"]) == (20, 3, 4)
    empties = [w for w in got["wgs"] if w["nrows"] == 0]
    assert len(empties) == 1 and empties[0]["fmt1"] == 1
    for w in empties:
        assert w["ngroups"] == 0 and w["T"] == 0 and w["nfast"] == 0


def test_seam_and_clamped_slots(E):
    # K = 4096: 2 groups per row, 28 per Q4_K slot.  The first workgroup owns the 32 Q|K rows
    # (64 groups): slot 0 (groups 0..27) crosses the Q|K seam at group 16, slot 1 (28..55) lies inside K
    # at offset 12, slot 2 (56..83) runs past the workgroup's last group and is clamped
    got = check(E, [Q4, Q4, Q6], [8, 24, 16], 4096, 2)
    w = got["wgs"][0]
    assert (w["r0"], w["nrows"], w["ngroups"], w["T"]) == (0, 32, 64, 3)
    pro = w["pro"]
    assert pro[0]["seam"] and not pro[0]["fast"] and pro[0]["seg"] == 0
    assert pro[1]["fast"] and pro[1]["seg"] == 1 and pro[1]["off"] == 12
    assert not pro[2]["fast"] and not pro[2]["seam"]
    assert w["nfast"] == 0
    # the Q6_K workgroup: 16 rows = 32 groups of 14 per slot, offsets within the V segment
    v = got["wgs"][1]
    assert v["fmt1"] == 1 and v["T"] == 3 and v["nfast"] == 2
    assert [p["off"] for p in v["pro"][:3]] == [0, 14, 28] and all(p["seg"] == 2 for p in v["pro"][:3])
