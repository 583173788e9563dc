"""The device pooling kernel (embed_pool_kernel in csrc/kernels/embed_pool.hip) through the raw op
`_engine.embed_pool`, against the float64 oracle of its rule (tests/embed_oracle.py).

Rows are padded to ldx = d + 37 with the padding poisoned (1e30, then NaN), the rows behind n poisoned too,
and the outputs pre-filled with a sentinel, so an over-read shows in the result and an over-write in the
sentinel.  Metric: ||gpu - oracle||_2 on the unit vectors ("none": the largest relative row error
||gpu_row - oracle_row|| / ||oracle_row||), bound embed_oracle.GPU_TOL (measured; see there).

The kernel splits n rows over ceil(n / band) workgroups, band = ceil(n / 64): one row per workgroup up to
n = 64, two from 65, three from 129 -- the boundaries tested besides the issue's.  A sum split over two
launches associates differently from the single launch (the kernel's comment), so chunked accumulation is
compared within GPU_TOL, not bit for bit; the same launch twice IS bit-identical.
"""
import numpy as np
import pytest
import torch

import embed_oracle as O

pytestmark = pytest.mark.gpu

TOL = O.GPU_TOL
PAD = 37
EXTRA = 2          # poisoned rows behind the n the launch may read
SENT = 777.0
EPS = 1e-5
MODE = {"none": 0, "mean": 1, "last": 3}


@pytest.fixture(scope="module")
def E():
    from aios_amd.runtime import native

    return native.require()


def stream():
    return torch.cuda.current_stream().cuda_stream


class Dev:
    """the device buffers of one sequence's pooling state and one launch's outputs"""

    def __init__(self, E, d, g, rows_out=0):
        self.E, self.d = E, d
        self.g = torch.from_numpy(np.asarray(g, np.float32)).cuda()
        self.acc = torch.full((d + PAD,), SENT, dtype=torch.float32, device="cuda")
        self.count = torch.full((4,), -5, dtype=torch.int32, device="cuda")
        self.out = torch.full((d + PAD,), SENT, dtype=torch.float32, device="cuda")
        self.rows = torch.full((rows_out + EXTRA, d), SENT, dtype=torch.float32, device="cuda")
        self.ws_bytes = E.embed_pool_ws_bytes(d)
        self.ws = torch.full((self.ws_bytes // 4,), float("nan"), dtype=torch.float32, device="cuda")
        self.counter = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.keep = []

    def fold(self, x, mode, first, final, poison=1e30):
        x = np.asarray(x, np.float32)
        n, d = x.shape
        buf = np.full((n + EXTRA, d + PAD), poison, np.float32)
        buf[:n, :d] = x
        t = torch.from_numpy(buf).cuda()
        self.keep.append(t)
        out = self.rows if mode == "none" else self.out
        self.E.embed_pool(t.data_ptr(), d + PAD, n, d, self.g.data_ptr(), EPS, self.acc.data_ptr(), self.count.data_ptr(),
                          MODE[mode], int(first), int(final), out.data_ptr(), self.ws.data_ptr(), self.ws_bytes,
                          self.counter.data_ptr(), stream())

    def result(self):
        torch.cuda.synchronize()
        out = self.out.cpu().numpy()
        assert np.all(out[self.d:] == SENT), "wrote past out[d]"
        assert np.all(self.acc.cpu().numpy()[self.d:] == SENT), "wrote past acc[d]"
        assert int(self.counter.cpu()[0]) == 0, "ticket not re-armed"
        return out[:self.d].copy()


def rows(n, d, seed, scale=1.0):
    return (np.random.default_rng(seed).standard_normal((n, d)) * scale).astype(np.float32)


def weight(d, seed=99):
    return (1.0 + 0.5 * np.random.default_rng(seed).standard_normal(d)).astype(np.float32)


def dist(name, got, want):
    assert np.all(np.isfinite(got)), f"{name}: non-finite output"
    e = float(np.linalg.norm(got.astype(np.float64) - want))
    print(f"embed_pool {name}: ||gpu - oracle|| = {e:.3e}")
    return e


def check(E, name, x, g, mode="mean", poisons=(1e30, float("nan"))):
    want = O.embed(x, g, EPS, mode)
    for p in poisons:
        dev = Dev(E, x.shape[1], g)
        dev.fold(x, mode, True, True, p)
        got = dev.result()
        e = dist(f"{name} {mode} pad={p}", got, want)
        assert e <= TOL, f"{name}: distance {e:.3e} above {TOL:.1e}"
        assert int(dev.count.cpu()[0]) == (1 if mode == "last" else x.shape[0])
    return got


@pytest.mark.parametrize("n", [1, 2, 3])
@pytest.mark.parametrize("d", [64, 256, 2048, 5120, 8192])
def test_widths(E, d, n):
    check(E, f"d={d} n={n}", rows(n, d, d + n), weight(d))


@pytest.mark.parametrize("n", [63, 64, 65, 128, 129, 255, 256, 257, 2048])
@pytest.mark.parametrize("d", [256, 4096])
def test_row_counts(E, d, n):
    check(E, f"d={d} n={n}", rows(n, d, 7 * d + n), weight(d), poisons=(float("nan"),))


@pytest.mark.parametrize("d", [192, 1024, 6144])
def test_other_multiples_of_64(E, d):
    check(E, f"d={d} n=5", rows(5, d, d), weight(d))


@pytest.mark.parametrize("n", [2, 66, 300])
def test_chunked_accumulation(E, n):
    d = 1024
    x, g = rows(n, d, n), weight(d)
    want = O.embed(x, g, EPS, "mean")
    single = Dev(E, d, g)
    single.fold(x, "mean", True, True)
    one = single.result()
    for n1 in sorted({1, n // 2, n - 1}):
        dev = Dev(E, d, g)
        dev.fold(x[:n1], "mean", True, False)
        torch.cuda.synchronize()
        assert np.all(dev.out.cpu().numpy() == SENT), "a non-final launch wrote the output"
        assert int(dev.count.cpu()[0]) == n1
        dev.fold(x[n1:], "mean", False, True, float("nan"))
        got = dev.result()
        assert int(dev.count.cpu()[0]) == n
        e = dist(f"chunked n={n} n1={n1}", got, want)
        e1 = dist(f"chunked n={n} n1={n1} vs single launch", got, one.astype(np.float64))
        assert e <= TOL and e1 <= TOL


def test_three_chunks_and_state_reset(E):
    d, g = 512, weight(512)
    x = rows(70, d, 3)
    dev = Dev(E, d, g)
    dev.fold(rows(9, d, 4), "mean", True, False)      # another sequence's leftovers: `first` must drop them
    dev.fold(x[:10], "mean", True, False)
    dev.fold(x[10:11], "mean", False, False)
    dev.fold(x[11:], "mean", False, True)
    assert dist("three chunks", dev.result(), O.embed(x, g, EPS, "mean")) <= TOL
    assert int(dev.count.cpu()[0]) == 70


@pytest.mark.parametrize("n,d", [(257, 256), (65, 4096), (3, 8192)])
def test_deterministic(E, n, d):
    x, g = rows(n, d, 5), weight(d)
    outs = []
    for _ in range(2):
        dev = Dev(E, d, g)
        dev.fold(x, "mean", True, True)
        outs.append(dev.result())
    assert outs[0].tobytes() == outs[1].tobytes()


@pytest.mark.parametrize("scale", [1e-3, 1e3])
def test_scaled_rows(E, scale):
    check(E, f"scale={scale}", rows(66, 2048, 8, scale), weight(2048))


def test_mixed_scales_count_equally(E):
    # every row is normed before the sum: a 1e3 row weighs what a 1e-3 row does
    x = rows(6, 1024, 9)
    x[::2] *= 1e3
    x[1::2] *= 1e-3
    check(E, "mixed scales", x, weight(1024))


def test_outlier(E):
    x = rows(5, 4096, 10)
    x[2, 1234] = 1e4
    check(E, "outlier", x, weight(4096))


def test_zero_row_among_others(E):
    x = rows(5, 512, 11)
    x[3] = 0.0
    check(E, "zero row", x, weight(512))


@pytest.mark.parametrize("mode", ["mean", "last"])
@pytest.mark.parametrize("n,d", [(1, 64), (67, 2048)])
def test_all_zero_rows(E, mode, n, d):
    dev = Dev(E, d, weight(d))
    dev.fold(np.zeros((n, d), np.float32), mode, True, True)
    got = dev.result()
    assert np.all(got == 0.0), "all-zero rows must give exact zeros"


@pytest.mark.parametrize("n", [1, 65])
def test_last(E, n):
    d = 2048
    x, g = rows(n, d, 12), weight(d)
    x[:n - 1] = np.nan  # the earlier rows must not reach the output
    want = O.embed(x, g, EPS, "last")
    dev = Dev(E, d, g)
    dev.fold(x, "last", False, True, float("nan"))
    assert dist(f"last n={n}", dev.result(), want) <= TOL


@pytest.mark.parametrize("n,d", [(1, 64), (3, 5120), (65, 256), (130, 4096)])
def test_none(E, n, d):
    x, g = rows(n, d, 13), weight(d)
    x[n // 2] *= 1e3
    want = O.embed(x, g, EPS, "none")
    dev = Dev(E, d, g, rows_out=n)
    dev.fold(x, "none", True, True, float("nan"))
    torch.cuda.synchronize()
    got = dev.rows.cpu().numpy()
    assert np.all(got[n:] == SENT), "wrote past row n"
    assert np.all(dev.out.cpu().numpy() == SENT) and np.all(dev.acc.cpu().numpy() == SENT), "none touched the pooled state"
    assert np.all(np.isfinite(got[:n]))
    rel = np.linalg.norm(got[:n].astype(np.float64) - want, axis=1) / np.linalg.norm(want, axis=1)
    print(f"embed_pool none n={n} d={d}: max relative row error = {rel.max():.3e}")
    assert rel.max() <= TOL


@pytest.mark.parametrize("d", [0, 32, 100, 8192 + 64, 8200])
def test_refused_widths_launch_nothing(E, d):
    dev = Dev(E, 64, weight(64))
    x = torch.zeros((2, max(d, 64) + PAD), dtype=torch.float32, device="cuda")
    with pytest.raises(RuntimeError, match="multiple of 64"):
        E.embed_pool(x.data_ptr(), max(d, 64) + PAD, 2, d, dev.g.data_ptr(), EPS, dev.acc.data_ptr(), dev.count.data_ptr(), 1, 1, 1,
                     dev.out.data_ptr(), dev.ws.data_ptr(), dev.ws_bytes, dev.counter.data_ptr(), stream())
    torch.cuda.synchronize()
    assert np.all(dev.out.cpu().numpy() == SENT) and np.all(dev.acc.cpu().numpy() == SENT)


def test_refused_rows_mode_and_workspace(E):
    d = 64
    dev = Dev(E, d, weight(d))
    x = torch.zeros((4, d + PAD), dtype=torch.float32, device="cuda")

    def go(n=2, mode=1, ws_bytes=dev.ws_bytes, ldx=d + PAD):
        E.embed_pool(x.data_ptr(), ldx, n, d, dev.g.data_ptr(), EPS, dev.acc.data_ptr(), dev.count.data_ptr(), mode, 1, 1,
                     dev.out.data_ptr(), dev.ws.data_ptr(), ws_bytes, dev.counter.data_ptr(), stream())

    for kw in (dict(n=0), dict(n=2049), dict(mode=2), dict(ws_bytes=dev.ws_bytes - 4), dict(ldx=d - 1)):
        with pytest.raises(RuntimeError):
            go(**kw)
    torch.cuda.synchronize()
    assert np.all(dev.out.cpu().numpy() == SENT)
