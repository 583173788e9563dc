"""The decode and prefill attention kernels against the float64 oracle (tests/attention_oracle.py) on
inputs built to expose them: a peaked softmax (one needle key holds the mass, V rows independent, so a
wrong key, head or mask is an O(1) error), score ramps (the running maximum moves in every pass, or
never, or once from one lane), non-finite or tempting data in every key position no live key owns, and
the launch modes and knobs nothing else runs.

Tolerance, both kernels: |out - ref| <= c * mag + 1e-6 with mag = sum_k p_k |v_kd| / sum_k p_k from the
oracle -- derived, not measured:
  decode   c = 2^-16: fp32 P.V and fp32 accumulation over at most 64 partials plus v_exp_f32's error,
           with margin; the bf16 output (out16) is checked bit for bit against the rounded fp32 output.
  prefill  c = 2^-7: P rounded to bf16 and the output rounded to bf16.  (bf16's unit roundoff is 2^-8,
           so 2^-7 is the worst-case sum of the two, not twice it; the observed ratio stays well inside
           because the rounding errors of P average out and a needle's own weight is exactly 1.)
Largest observed |err| / mag on an MI355X (this module's cases; every test prints its own, pytest -s):
  decode   1.7e-6 (bound 1.5e-5); out16 3.7e-3 (bound 2^-8 + 2^-16 = 3.9e-3)
  prefill  5.3e-3 (bound 7.8e-3), on the ascending ramp, where hundreds of rounded weights share the mass
"""
import math

import pytest
import torch

import attention_oracle as O

pytestmark = pytest.mark.gpu

C_DECODE = 2.0 ** -16
C_PREFILL = 2.0 ** -7


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


def check(out, ref, mag, c, what):
    """finite and within c * mag + 1e-6 everywhere; prints the largest |err| / mag (pytest -s shows it)"""
    out = out.double()
    assert bool(torch.isfinite(out).all()), (what, "non-finite output", int((~torch.isfinite(out)).sum()))
    err = (out - ref).abs()
    print(f"{what}: max |err| / mag = {float((err / (mag + 1e-30)).max()):.3e} (bound {c:.3e})")
    bad = err > c * mag + 1e-6
    assert not bool(bad.any()), (what, int(bad.sum()), float(err.max()), float((err / (c * mag + 1e-6)).max()))


def launch_decode(E, c, kp, vp, bt, split=0, want16=False, launches=2, **kw):
    """Launches attn_decode `launches` times on pools kp / vp (CPU tensors) and returns out [B, H, hd]
    (fp32, or the bf16 out16); asserts the arrival counters re-armed to zero after every launch."""
    B, (H, hd) = len(c.lens), c.q.shape[1:]
    Hkv = c.kraw.shape[1]
    kd, vd = kp.cuda(), vp.cuda()
    btd = bt.cuda() if bt is not None else None
    q = c.q.cuda()
    seq = torch.tensor(c.lens, dtype=torch.int32, device="cuda")
    slot = torch.tensor(c.slot, dtype=torch.int32, device="cuda")
    nch = c.max_ctx // E.ATTN_CHUNK
    opart = torch.full((B, H, nch, hd), float("nan"), device="cuda")
    ml = torch.full((B, H, nch, 2), float("nan"), device="cuda")
    out = torch.empty(B, H, hd, device="cuda")
    out16 = torch.empty(B, H, hd, dtype=torch.bfloat16, device="cuda")
    cnt = torch.zeros(B, H, dtype=torch.int32, device="cuda")
    for _ in range(launches):
        out.fill_(float("nan"))
        out16.fill_(float("nan"))
        E.attn_decode(q.data_ptr(), kd.data_ptr(), vd.data_ptr(), seq.data_ptr(), slot.data_ptr(), B, H, Hkv, hd,
                      c.max_ctx, nch, c.scale, opart.data_ptr(), ml.data_ptr(), out.data_ptr(), cnt.data_ptr(), stream(),
                      split, btd.data_ptr() if btd is not None else 0, 0, kv_fp8=int(c.fp8), k_scale=c.sk, v_scale=c.sv,
                      out16=out16.data_ptr() if want16 else 0, **kw)
        torch.cuda.synchronize()
        assert int(cnt.abs().sum()) == 0, "arrival counters not re-armed"
    if want16:
        assert bool(out.isnan().all()), "out16 set: the fp32 output must stay untouched"
        return out16.cpu()
    return out.cpu()


def check_decode(c, out, what, c_tol=C_DECODE, rows=None):
    for b in (range(len(c.lens)) if rows is None else rows):
        ref, mag = c.ref(slice(b, b + 1), c.slot[b], c.lens[b])
        check(out[b:b + 1], ref, mag, c_tol, f"{what} row {b} len {c.lens[b]}")


# ---------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize("shuffle", [False, True], ids=["identity", "shuffled"])
@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("family", O.DECODE_FAMILIES)
@pytest.mark.parametrize("lens,max_ctx", O.DECODE_LENS)
@pytest.mark.parametrize("hd,H,Hkv", O.DECODE_LAYOUTS)
def test_decode_adversarial(E, hd, H, Hkv, lens, max_ctx, family, fp8, shuffle):
    """Every head layout x edge length x family x pool type x table, at the launcher's defaults, with
    every dead key position poisoned: finite output within the fp32 bound, counters re-armed."""
    c = O.decode_case(family, hd, H, Hkv, lens, max_ctx, fp8, seed=21)
    kp, vp, bt, _ = O.pools(c, shuffle, seed=22, mode="poison")
    check_decode(c, launch_decode(E, c, kp, vp, bt), f"decode {family}")


KNOBS = [("env", "AIOS_ATTN_SHORT_P", "2"), ("env", "AIOS_ATTN_SHORT_P", "4"), ("env", "AIOS_ATTN_PPW", "2"),
         ("env", "AIOS_ATTN_XCD", "0"), ("arg", "combine_trips", 2), ("arg", "kv_nt", 0), ("arg", "short_len", 0),
         ("arg", "short_len", 4096), ("arg", "kv_tail", 0)]


@pytest.mark.parametrize("family", ["peaked-127", "ascending"])
@pytest.mark.parametrize("kind,name,value", KNOBS, ids=[f"{n}={v}" for _, n, v in KNOBS])
def test_decode_knobs(E, monkeypatch, kind, name, value, family):
    """One launcher knob at a time, one short-mode and one long-mode row.  kv_tail = 0 loads the dead
    keys of the last block (ops.h: they must be finite), so it runs on decoys -- the best-scoring K row
    of the case with V = 100 in every dead position -- instead of poison: the mask alone keeps them out."""
    hd, H, Hkv, lens, max_ctx = O.DECODE_KNOB
    c = O.decode_case(family, hd, H, Hkv, lens, max_ctx, False, seed=23)
    kw = {}
    if kind == "env":
        monkeypatch.setenv(name, value)
    else:
        kw[name] = value
    if name == "kv_tail":
        krow = c.kraw[1, :, 127 if family.startswith("peaked") else max_ctx - 1]
        kp, vp, bt, _ = O.pools(c, True, seed=24, mode="decoy", krow=krow)
    else:
        kp, vp, bt, _ = O.pools(c, True, seed=24, mode="poison")
    check_decode(c, launch_decode(E, c, kp, vp, bt, **kw), f"decode {name}={value} {family}")


@pytest.mark.parametrize("family", ["peaked-last", "ascending"])
@pytest.mark.parametrize("hd,H,Hkv,lens,max_ctx", O.DECODE_WIDE, ids=["34wg", "64wg"])
def test_decode_more_than_32_partials(E, hd, H, Hkv, lens, max_ctx, family):
    """split = 4096 gives 64 workgroups per head set, of which ceil(len / 128) = 34 / 64 are active: the
    two-trip combine's `nact > 32` path (asserted from the plan, so a changed plan fails here loudly)."""
    split = 4096
    p_long = max(1, min(max_ctx // 128, split // E.ATTN_CHUNK))
    active = min(-(-lens[0] // 128), p_long)
    assert active > 32 and active == {4225: 34, 8192: 64}[lens[0]]
    c = O.decode_case(family, hd, H, Hkv, lens, max_ctx, False, seed=25)
    kp, vp, bt, _ = O.pools(c, True, seed=26, mode="poison")
    check_decode(c, launch_decode(E, c, kp, vp, bt, split=split), f"decode {active} partials {family}")


@pytest.mark.parametrize("family", ["peaked-127", "ascending"])
def test_decode_out16_and_write_through(E, family):
    """The same launch three ways -- fp32 out, bf16 out16, fp32 with write-through stores -- over a
    short-mode row (no combine) and a long-mode row (combine): out16 is the RNE rounding of out bit for
    bit, out_wt changes no bit."""
    hd, H, Hkv, lens, max_ctx = O.DECODE_KNOB
    c = O.decode_case(family, hd, H, Hkv, lens, max_ctx, False, seed=27)
    kp, vp, bt, _ = O.pools(c, True, seed=28, mode="poison")
    out = launch_decode(E, c, kp, vp, bt)
    check_decode(c, out, f"decode out {family}")
    o16 = launch_decode(E, c, kp, vp, bt, want16=True)
    assert torch.equal(o16.view(torch.int16), out.to(torch.bfloat16).view(torch.int16))
    check_decode(c, o16, f"decode out16 {family}", C_DECODE + 2.0 ** -8)
    owt = launch_decode(E, c, kp, vp, bt, out_wt=1)
    assert torch.equal(owt.view(torch.int32), out.view(torch.int32))


def test_decode_empty_row_leaves_the_rest_alone(E):
    """launch_attn_decode's contract (ops.h): seq_len >= 1 -- the engine uploads pos + 1 everywhere.  An
    empty row's own output is unspecified, but it must not disturb its neighbours or the counters."""
    c = O.decode_case("peaked-last", 128, 32, 8, [0, 5], 256, False, seed=29)
    kp, vp, bt, _ = O.pools(c, True, seed=30, mode="poison")
    out = launch_decode(E, c, kp, vp, bt)
    check_decode(c, out, "decode [0, 5]", rows=[1])


# ---------------------------------------------------------------------------------------- prefill
def launch_prefill(E, c, kp, vp, bt):
    T, H, hd = c.q.shape
    kd, vd, btd = kp.cuda(), vp.cuda(), bt.cuda() if bt is not None else None
    q = c.q.cuda()
    out = torch.full((T, H * hd), float("nan"), dtype=torch.bfloat16, device="cuda")
    E.attn_prefill(q.data_ptr(), kd.data_ptr(), vd.data_ptr(), 1, c.start, T, H, c.kraw.shape[1], hd, c.max_ctx,
                   c.scale, out.data_ptr(), H * hd, stream(), btd.data_ptr() if btd is not None else 0,
                   kv_fp8=int(c.fp8), k_scale=c.sk, v_scale=c.sv)
    torch.cuda.synchronize()
    return out.cpu().view(T, H, hd)


def check_prefill(c, out, what):
    ref, mag = c.ref(slice(0, c.T), 1, c.start + c.T)
    check(out, ref, mag, C_PREFILL, what)


@pytest.mark.parametrize("fp8", [False, True], ids=["bf16", "fp8"])
@pytest.mark.parametrize("family", O.PREFILL_FAMILIES)
@pytest.mark.parametrize("start,T", O.PREFILL_CASES)
@pytest.mark.parametrize("H,Hkv,hd", O.PREFILL_LAYOUTS)
def test_prefill_adversarial(E, H, Hkv, hd, start, T, family, fp8):
    """Every layout x (start, T) edge x family x pool type on a shuffled table with everything at or
    past start + T poisoned.  peaked: the diagonal is the needle and key qpos + 1 -- the best raw score
    of the row -- must stay masked; the last tile's dead V rows must not reach the MFMA."""
    c = O.prefill_case(family, H, Hkv, hd, start, T, fp8, seed=31)
    kp, vp, bt, _ = O.pools(c, True, seed=32, mode="poison")
    check_prefill(c, launch_prefill(E, c, kp, vp, bt), f"prefill {family} ({start}, {T})")


@pytest.mark.parametrize("family", O.PREFILL_FAMILIES)
def test_prefill_chunked(E, family):
    """[0, 150) in one launch, and as [0, 70) then [70, 150) (the second chunk written only after the
    first ran: poison from key 70 on for the first launch): each against the oracle."""
    H, Hkv, hd = 32, 8, 128
    for start, T in ((0, 150), (0, 70), (70, 80)):
        c = O.prefill_case(family, H, Hkv, hd, start, T, False, seed=33)
        kp, vp, bt, _ = O.pools(c, True, seed=34, mode="poison")
        check_prefill(c, launch_prefill(E, c, kp, vp, bt), f"prefill chunk ({start}, {T}) {family}")
