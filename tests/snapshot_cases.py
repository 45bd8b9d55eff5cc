"""Hand-built micro-chains for the snapshot rules S1-S8, each with its expected arrays written out,
plus a fuzzed chain generator.  Shared by test_snapshots.py (CPU) and test_snapshots_gpu.py."""
import numpy as np
import pandas as pd

DAY = "2023-03-01 "
YEAR_NS = 365 * 86400 * 10**9
EXPIRY = {"02mar23": pd.Timestamp("2023-03-02 08:00"), "10mar23": pd.Timestamp("2023-03-10 08:00"),
          "01mar23": pd.Timestamp("2023-03-01 10:02")}
NAN = np.nan


def chain(rows):
    """rows: (symbol, 'HH:MM:SS', iv, underlying_price, strike, callput); time_to_maturity = (E - date) / YEAR."""
    out = []
    for sym, hms, iv, up, k, cp in rows:
        d = pd.Timestamp(DAY + hms)
        lab = sym.split("-")[1].lower() if sym.count("-") == 3 else "02mar23"
        E = EXPIRY.get(lab, EXPIRY["02mar23"])
        out.append({"symbol": sym, "date": d, "iv": iv, "underlying_price": up,
                    "time_to_maturity": (E.value - d.value) / YEAR_NS, "strike": k, "callput": cp,
                    "interest_rate": 0.0, "volume": 1.0})
    return pd.DataFrame(out)


def _c(k, hms, iv, up=25000.0, exp="02mar23", und="btc"):
    return (f"{und}-{exp}-{int(k)}-c", hms, iv, up, float(k), "c")


def _p(k, hms, iv, up=25000.0, exp="02mar23", und="btc"):
    return (f"{und}-{exp}-{int(k)}-p", hms, iv, up, float(k), "p")


# name -> (frame, expected): expected keys per underlying 'btc' unless a dict of underlyings; sigma [B][nT][nK]
CASES = {
    # S5: both sides -> OTM; strike == F -> call; F is the PUT row's underlying price (the call row says 25001)
    "otm": (chain([_c(24000, "10:00:00", .50, 25001), _c(25000, "10:00:00", .51, 25001), _c(26000, "10:00:00", .52, 25001),
                   _p(24000, "10:00:00", .60), _p(25000, "10:00:00", .61), _p(26000, "10:00:00", .62)]),
            dict(sigma=[[[.60, .51, .52]]], quotes=[3], spot=[25000.0])),
    # S5: only one side present
    "one_side": (chain([_c(24000, "10:00:00", .50, 24990), _p(26000, "10:00:00", .70, 25010)]),
                 dict(sigma=[[[.50, .70]]], quotes=[2], spot=[24990.0])),
    # S3: a strike listed in one expiry only
    "missing_strike": (chain([_c(26000, "10:00:00", .50), _c(27000, "10:00:00", .51),
                              _c(27000, "10:00:00", .41, exp="10mar23")]),
                       dict(sigma=[[[.50, .51], [NAN, .41]]], quotes=[3], spot=[25000.0])),
    # S5: several rows in one minute -> the last in date order; equal timestamps -> the later input row
    "last_wins": (chain([_c(26000, "10:00:00", .50), _c(26000, "10:00:40", .55), _c(26000, "10:00:40", .56, 25005),
                         _c(26000, "10:00:40", .57, 25007), _c(26000, "10:00:20", .58)]),
                  dict(sigma=[[[.57]]], quotes=[1], spot=[25007.0])),
    # S4: seconds are floored, t0 is the first minute
    "seconds": (chain([_c(26000, "10:00:30", .50), _c(26000, "10:01:30", .51)]),
                dict(sigma=[[[.50]], [[.51]]], quotes=[1, 1], spot=[25000.0, 25000.0])),
    # S5: a contract that starts late is NaN before its first row
    "late_start": (chain([_c(26000, "10:00:00", .50), _c(26000, "10:01:00", .51), _c(26000, "10:02:00", .52),
                          _c(27000, "10:02:00", .60, 25002)]),
                   dict(sigma=[[[.50, NAN]], [[.51, NAN]], [[.52, .60]]], quotes=[1, 1, 2], spot=[25000.0] * 3)),
    # S6: expiry 01mar23 passes at 10:02 -> its row is NaN from that minute on; T stays analytic
    "expiring": (chain([_c(26000, f"10:0{m}:00", .30 + m / 100, exp="01mar23") for m in range(4)]
                       + [_c(26000, f"10:0{m}:00", .50 + m / 100, 25100) for m in range(4)]),
                 dict(sigma=[[[.30], [.50]], [[.31], [.51]], [[NAN], [.52]], [[NAN], [.53]]], quotes=[2, 2, 1, 1],
                      spot=[25000.0, 25000.0, 25100.0, 25100.0])),
    # S4/S7: a minute without rows -> quotes 0, spot NaN (and no rows in to_frame)
    "empty_minute": (chain([_c(26000, "10:00:00", .50), _c(26000, "10:02:00", .52)]),
                     dict(sigma=[[[.50]], [[NAN]], [[.52]]], quotes=[1, 0, 1], spot=[25000.0, NAN, 25000.0])),
    # S5: a NaN iv is absent: the put would be OTM (24000 < F) but is NaN -> the call
    "nan_iv": (chain([_c(24000, "10:00:00", .50, 25003), _p(24000, "10:00:00", NAN)]),
               dict(sigma=[[[.50]]], quotes=[1], spot=[25003.0])),
    # S1: unparsable symbol and a side that is neither c nor p are skipped and counted
    "skipped": (chain([_c(26000, "10:00:00", .50), ("garbage", "10:00:00", .9, 1.0, 1.0, "c"),
                       ("btc-02mar23-27000-c", "10:00:00", .9, 25000.0, 27000.0, "straddle"),
                       ("btc-02mar23-2x000-c", "10:00:00", .9, 25000.0, 27000.0, "c")]),
                dict(sigma=[[[.50]]], quotes=[1], spot=[25000.0], skipped=3)),
    # S1: two underlyings in one frame (ETH parsed case-insensitively); each gets its own axes and window
    "two_underlyings": (chain([_c(26000, "10:00:00", .50), ("ETH-02MAR23-1800-P", "10:01:00", .70, 1700.0, 1800.0, "P")]),
                        {"btc": dict(sigma=[[[.50]]], quotes=[1], spot=[25000.0]),
                         "eth": dict(sigma=[[[.70]]], quotes=[1], spot=[1700.0])}),
}


def expected(name):
    exp = CASES[name][1]
    return exp if "btc" in exp else {"btc": exp}


def too_many_expiries():
    rows = []
    for i in range(33):
        E = pd.Timestamp("2023-03-02") + pd.Timedelta(days=i)
        d = pd.Timestamp(DAY + "10:00:00")
        rows.append({"symbol": f"btc-e{i:02d}-25000-c", "date": d, "iv": .5, "underlying_price": 25000.0,
                     "time_to_maturity": (E.value - d.value) / YEAR_NS, "strike": 25000.0, "callput": "c"})
    return pd.DataFrame(rows)


def fuzz_chain(seed, n_min=45, expiries=(1.0 / 24 / 3, 1, 5, 20), strikes=(23000, 24000, 24500, 25000, 25500, 26000, 27000)):
    """A random minute-level chain: unlisted strikes per expiry, random leading gaps, duplicate minutes (with seconds),
    mixed-case callput, NaN ivs, empty minutes and an expiry that passes inside the window."""
    r = np.random.default_rng(seed)
    t0 = pd.Timestamp("2023-03-01 09:00") + pd.Timedelta(seconds=int(r.integers(0, 30)))
    holes = set(r.choice(n_min, 3, replace=False).tolist())                       # minutes with no rows at all
    rows = []
    for days in expiries:
        E = pd.Timestamp("2023-03-01 09:00") + pd.Timedelta(days=days)
        lab = E.strftime("%d%b%y").lower() + (f"h{E.hour}" if days < 1 else "")
        for k in strikes:
            if r.random() < 0.2:
                continue                                                         # unlisted at this expiry
            for side in "cp":
                start = int(r.integers(0, n_min // 3)) if r.random() < 0.4 else 0
                for m in range(start, n_min):
                    if m in holes or r.random() < 0.05:
                        continue
                    reps = 2 if r.random() < 0.1 else 1
                    for _ in range(reps):
                        d = t0 + pd.Timedelta(minutes=m, seconds=int(r.integers(0, 30)) if reps > 1 else 0)
                        F = 25000.0 + 30 * np.sin(m / 7.0) + days
                        iv = np.nan if r.random() < 0.03 else 0.4 + 0.1 * r.random() + (0.05 if side == "p" else 0)
                        cp = {"c": ["c", "C", "call", "Call"], "p": ["p", "P", "put", "PUT"]}[side][int(r.integers(0, 4))]
                        rows.append({"symbol": f"btc-{lab}-{k}-{side}", "date": d, "iv": iv, "underlying_price": F,
                                     "time_to_maturity": (E.value - d.value) / YEAR_NS, "strike": float(k), "callput": cp})
    df = pd.DataFrame(rows)
    return df.iloc[r.permutation(len(df))].reset_index(drop=True)               # input order is not date order


UNDERLYINGS = ["btc", "eth", "sol", "xrp"]


def big_chain(n_und=2, nT=12, nK=48, minutes=3781, seed=0, unlisted=0.1):
    """A full-size minute chain as one long frame (rows grouped by contract, date-sorted): n_und underlyings x nT
    expiries x nK strikes x 2 sides x `minutes` minutes, ~`unlisted` of the strikes unlisted per expiry, and the nearest
    expiry passing in the middle of the window (its contracts stop quoting there)."""
    r = np.random.default_rng(seed)
    t0 = pd.Timestamp("2023-03-01 00:00").value
    d_ns = t0 + 60 * 10**9 * np.arange(minutes, dtype=np.int64)
    syms, lens, cols = [], [], {k: [] for k in ("date", "iv", "underlying_price", "time_to_maturity", "strike", "callput")}
    for u in range(n_und):
        s0 = [25000.0, 1800.0, 22.0, 0.4][u % 4]
        spot = s0 * np.exp(np.cumsum(r.normal(0, 2e-4, minutes)))
        strikes = s0 * np.linspace(0.7, 1.3, nK)
        for e in range(nT):
            E = t0 + (minutes // 2) * 60 * 10**9 if e == 0 else t0 + e * 7 * 86400 * 10**9
            live = d_ns < E
            n = int(live.sum())
            ttm = (E - d_ns[live]) / YEAR_NS
            fwd = spot[live] * np.exp(0.03 * ttm)
            for k in strikes:
                if e > 0 and r.random() < unlisted:
                    continue
                base = 0.5 + 0.2 * np.log(k / fwd) ** 2
                for side in "cp":
                    syms.append(f"{UNDERLYINGS[u % 4]}-x{e:02d}-{k:.4f}-{side}")
                    lens.append(n)
                    cols["date"].append(d_ns[live]); cols["iv"].append(base + (0.03 if side == "p" else 0.0))
                    cols["underlying_price"].append(fwd); cols["time_to_maturity"].append(ttm)
                    cols["strike"].append(np.full(n, k)); cols["callput"].append(np.full(n, side, dtype=object))
    iv = np.concatenate(cols["iv"])
    iv = iv + r.normal(0, 0.002, iv.size)
    return pd.DataFrame({"symbol": np.repeat(np.array(syms, dtype=object), lens),
                         "date": pd.DatetimeIndex(np.concatenate(cols["date"]).view("datetime64[ns]")),
                         "iv": iv, "underlying_price": np.concatenate(cols["underlying_price"]),
                         "time_to_maturity": np.concatenate(cols["time_to_maturity"]),
                         "strike": np.concatenate(cols["strike"]), "callput": np.concatenate(cols["callput"])})
