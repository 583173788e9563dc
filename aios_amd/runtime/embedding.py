"""The text-embedding rule on the host (csrc/ops.h EmbedPoolArgs is the device's; tests/embed_oracle.py the
float64 oracle): hidden rows x[t] -> h[t] = x[t] * g / sqrt(mean(x[t]^2) + eps), the model's final RMSNorm;
"mean": p = mean_t h[t], "last": p = h[T-1], result p / ||p||_2 (an exactly zero p stays the zero vector);
"none": the rows h themselves, not L2-normalised.  llama.cpp's --embedding output for a causal model."""
from __future__ import annotations

import numpy as np

# GGUF's {arch}.pooling_type codes, the engines' `pooling` argument
POOLING = {"none": 0, "mean": 1, "last": 3}
POOLING_NAMES = {v: k for k, v in POOLING.items()}
MAX_INPUTS = 64  # inputs per /v1/embeddings request


def pooling_code(pooling) -> int:
    if isinstance(pooling, str):
        if pooling not in POOLING:
            raise ValueError(f"pooling must be one of {sorted(POOLING)}, got {pooling!r}")
        return POOLING[pooling]
    if int(pooling) not in POOLING_NAMES:
        raise ValueError(f"pooling code must be one of {sorted(POOLING_NAMES)}, got {pooling!r}")
    return int(pooling)


def normed_rows(x: np.ndarray, g: np.ndarray, eps: float) -> np.ndarray:
    x = np.asarray(x, np.float64)
    return x * np.asarray(g, np.float64) / np.sqrt((x * x).mean(-1, keepdims=True) + float(eps))


def unit(p: np.ndarray) -> np.ndarray:
    p = np.asarray(p, np.float64)
    big = np.abs(p).max() if p.size else 0.0
    if big == 0.0:
        return np.zeros_like(p)
    p = p / big
    return p / np.sqrt((p * p).sum())
