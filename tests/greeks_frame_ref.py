"""Plain NumPy reference for the Greeks epilogue of the 1-D eval kernel and of the fused frame pass in multi-symbol CSR
batches.  TEST INFRASTRUCTURE ONLY.  Only the epilogue is restated: the forward fill of the strike / rate / put-code
columns and the Black-Scholes formulas (oracle/greeks_oracle.py) on channel values the caller supplies."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import greeks_oracle as G  # noqa: E402

GREEKS = ("delta", "gamma", "theta", "vega", "rho")


def ffill_rows(pos, src_off, q_off, valid):
    """Per output row: flat index of the symbol's last source row at or before it (by lattice position) whose `valid` byte
    is set, or -1.  Never a row of another symbol."""
    idx = np.full(int(q_off[-1]), -1, np.int64)
    for s in range(len(src_off) - 1):
        a, b = int(src_off[s]), int(src_off[s + 1])
        last = np.full(int(q_off[s + 1] - q_off[s]), -1, np.int64)
        for j in range(a, b):                       # ascending positions: a later valid row overwrites from its position on
            if valid[j]:
                last[int(pos[j]):] = j
        idx[int(q_off[s]):int(q_off[s + 1])] = last
    return idx


def epilogue(chan, pos, src_off, q_off, strike, rate=None, put=None):
    """chan = (iv, S, T) float64 [total_q] as the device returned them; strike / rate / put = (source column, validity) or
    None for an absent column.  Returns float64 [5, total_q]."""
    iv, S, T = chan
    n = int(q_off[-1])
    gather = lambda col, fill: np.where((i := ffill_rows(pos, src_off, q_off, col[1])) >= 0, col[0][np.maximum(i, 0)], fill)   # noqa: E731
    K = gather(strike, np.nan)                                            # no valid strike yet: NaN
    r = np.zeros(n) if rate is None else gather(rate, np.nan)             # absent column: 0.0; present but not valid yet: NaN
    code = np.zeros(n, np.int64) if put is None else gather((put[0].astype(np.int64), put[1]), 2)   # absent: a call; none valid: 2
    with np.errstate(all="ignore"):
        g = G.calculate_greeks(S, K, T, r, iv, code == 1)
    out = np.stack([g[k] for k in GREEKS])
    out[:, code == 2] = np.nan                                            # null option type: undefined
    return out
