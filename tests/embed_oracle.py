"""Float64 oracle of the text-embedding rule (csrc/ops.h EmbedPoolArgs), independent of the device kernel and
of runtime/embedding.py.  For hidden rows x[t], t = 0..T-1, of d floats, the norm weight g[d] and eps:

    h[t] = x[t] * g / sqrt(mean(x[t]^2) + eps)          the model's final RMSNorm (output_norm)
    "mean": p = (1 / T) sum_t h[t]      "last": p = h[T-1]      result p / ||p||_2
    "none": the T x d matrix h, not L2-normalised (llama.cpp's --pooling none)

A p that is exactly zero gives the zero vector, never NaN.  normed=True: the rows are h already (the engine's
own "none" rows): nothing is normed again, g and eps are not used; the oracle only averages and normalises.
"""
import numpy as np

# Tolerance of the device kernel against this oracle: ||gpu - oracle||_2 on the unit vectors ("none": the
# largest relative row error), four times the largest distance measured over every case of
# tests/test_embed_pool_gpu.py on an MI355X, 2.350e-07 (d = 1024, n = 300 folded as 150 + 150 rows against
# the single launch; against the oracle the largest was 1.898e-07, the same rows; profiles/embeddings.txt
# has every case).  The margin covers other boxes, compilers and math intrinsics.  It has to stay at or below
# 1e-3: dropping one of n independent N(0, 1) rows turns the unit result by about 1 / sqrt(n), 0.022 at the
# largest n tested (2048), so a measured distance near 1e-3 would be a bug, not a reason to raise it.
GPU_MEASURED = 2.350e-07
GPU_TOL = 4 * GPU_MEASURED
assert GPU_TOL <= 1e-3

POOLINGS = ("mean", "last", "none")


def normed(x, g, eps):
    x = np.asarray(x, np.float64)
    return x * np.asarray(g, np.float64) / np.sqrt(np.mean(x * x, axis=-1, keepdims=True) + np.float64(eps))


def unit(p):
    p = np.asarray(p, np.float64)
    n = np.sqrt(np.sum(p * p))
    return p / n if n > 0 else np.zeros_like(p)


def embed(x, g=None, eps=0.0, pooling="mean", normed_rows=False):
    """x [T][d] -> [d] ("mean", "last") or [T][d] ("none"), float64"""
    assert pooling in POOLINGS
    x = np.asarray(x, np.float64)
    assert x.ndim == 2 and x.shape[0] >= 1
    h = x if normed_rows else normed(x, g, eps)
    if pooling == "none":
        return h
    return unit(h.mean(axis=0) if pooling == "mean" else h[-1])
