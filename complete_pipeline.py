#!/usr/bin/env python3
"""Entry surface kept from the reference's ``complete_pipeline.py`` (reference :838-921): same class name,
same ``--task/--test/--symbols/--estimate/--setup-only`` flags, same result dictionaries.  Task 1 (IV
interpolation) runs on the MI355X engine -- many symbols per device launch through
``IVInterpolator.interpolate_batch`` instead of the reference's one-symbol-at-a-time loop
(:243-262) -- against a DB-less frame store (``--data-dir``).  The data bridge (reference :367-510, the pipeline's
own inline candle builder) and the 5-minute candle stage (:567-710) run on the engine too (SURVEY.md section 8f
ranks 3 and 4): all symbols of a stage in one device launch, tables ``minute_candles`` and ``reconstructed_candles``
in the same store."""
import argparse
import os
import sys
import time
from typing import List, Optional

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.append(os.path.join(ROOT, "src"))          # reference complete_pipeline.py:30

from config import get_config                          # noqa: E402
from interpolation.core import IVInterpolator          # noqa: E402  (reference :34)

import numpy as np                                      # noqa: E402
import pandas as pd                                     # noqa: E402

from iv_interpolation_amd.frame_store import FrameStore, synthetic_symbol   # noqa: E402

MINUTE_TABLE = "minute_candles"
CANDLE_TABLE = "reconstructed_candles"
SURFACE_TABLE = "iv_surfaces"
SMILE_TABLE = "iv_smiles"
ARBITRAGE_TABLE = "iv_arbitrage"
VOLINDEX_TABLE = "iv_volindex"
SVI_TABLE = "iv_svi"
DISTRIBUTION_TABLE = "iv_distribution"
CALENDAR_TABLE = "iv_calendar"
SSVI_TABLE = "iv_ssvi"
IMPLIED_TABLE = "iv_implied"
RISK_TABLE = "iv_risk"
EXPLAIN_TABLE = "iv_explain"
VAR_TABLE = "iv_var"
VAR_ATTRIB_TABLE = "iv_var_attrib"
HEDGE_TABLE = "iv_hedge"
WHATIF_TABLE = "iv_whatif"
VAR_CI_TABLE = "iv_var_ci"
VAR_W_TABLE = "iv_var_w"
SCENARIO_TABLE = "iv_scenarios"
PIPELINE_INLINE = 4                                     # engine strategy code of reference complete_pipeline.py:473-510


class CompleteOptimizedPipeline:
    def __init__(self, config, data_dir: Optional[str] = None, backend=None, bridge_backend=None, candle_backend=None,
                 seed: Optional[int] = None, surface_backend=None, implied_backend=None):
        self.config = config
        self._implied_backend = implied_backend          # None -> implied.HipImpliedBackend
        self._surface_backend = surface_backend          # None -> snapshots.HipBackend
        self.store = FrameStore(data_dir or config.data_dir)
        self._bridge_backend = bridge_backend            # None -> HipBridgeBackend / HipCandleBackend on first use
        self._candle_backend = candle_backend
        # the reference draws from the unseeded global NumPy generator; an explicit seed makes a run reproducible
        self.seed = int.from_bytes(os.urandom(4), "little") if seed is None else int(seed)
        self._rng_pos, self._rng_tail = 0, (0, 0)
        # the reference builds IVInterpolator() with defaults here (:49); config values are honoured instead
        # ... including `preserve_greeks` (reference config.py:46, read by nothing there): the interpolated rows then carry
        # the delta..rho columns the reference's schema reserves for them (src/database/schema.py:36-40)
        self.iv_interpolator = IVInterpolator(method=config.interpolation.method,
                                              min_points=config.interpolation.min_data_points, backend=backend,
                                              preserve_greeks=bool(getattr(config.interpolation, "preserve_greeks", False)))
        self.interrupted = False

    def setup_database_tables(self) -> dict:
        return {"success": True, "tables": ["trading_tickers", "interpolated_trading_tickers"], "root": self.store.root}

    def get_pipeline_status(self) -> dict:
        src = self.store.symbols()
        done = self.store.symbols("interpolated_trading_tickers")
        return {"source_symbols": len(src), "task1_symbols": len(done),
                "bridge_symbols": len(self.store.symbols(MINUTE_TABLE)), "task2_symbols": len(self.store.symbols(CANDLE_TABLE)),
                "source_rows": sum(len(self.store.read_symbol(s)) for s in src)}

    def run_task1_interpolation(self, symbols: List[str] = None, batch_id: int = None) -> dict:
        print("TASK 1: IV INTERPOLATION (MI355X engine)")
        print("-" * 40)
        if symbols is None:
            symbols = self.store.pending_symbols()
        if not symbols:
            return {"success": False, "error": "No symbols found for Task 1"}
        if batch_id is None:
            batch_id = int(time.time())
        start = time.time()
        ok = err = total_in = total_out = 0
        step = max(1, int(self.config.processing.symbols_per_batch))
        for a in range(0, len(symbols), step):
            if self.interrupted:
                break
            chunk = symbols[a:a + step]
            frames = [self.store.read_symbol(s) for s in chunk]
            results = self.iv_interpolator.interpolate_batch(frames)          # one device round trip per chunk
            for sym, src, out in zip(chunk, frames, results):
                if out is None:                                               # reference: status 'skipped'
                    err += 1
                    print(f"  {sym}: skipped (no valid data after interpolation)")
                    continue
                out = out.copy()
                out["is_interpolated"] = out["symbol"].isna()                 # recomputed as complete_pipeline.py:324
                n = self.store.write_output(sym, out, batch_id)
                ok += 1; total_in += len(src); total_out += n
                print(f"  {sym}: {len(src)} -> {n} rows")
        duration = time.time() - start
        print(f"\nTASK 1 COMPLETE: {duration:.1f}s, success {ok}, errors {err}, rows {total_in:,} -> {total_out:,}")
        return {"success": ok > 0, "batch_id": batch_id, "symbols_processed": ok, "total_input": total_in,
                "total_output": total_out, "duration": duration}

    def run_data_bridge(self, symbols: List[str] = None, batch_id: int = None) -> dict:
        """Reference :367-510.  One candle per interpolated row; base price = ``underlying or mark or index`` per row
        (:479, first TRUTHY value); all symbols in one launch, one generator stream in symbol order."""
        print("\nDATA BRIDGE: IV -> OHLCV CONVERSION (MI355X engine)")
        print("-" * 40)
        if symbols is None:                                                   # anti-join of :419-435
            done = set(self.store.symbols(MINUTE_TABLE))
            symbols = [s for s in self.store.symbols("interpolated_trading_tickers") if s not in done]
        if not symbols:
            return {"success": False, "error": "No symbols found for data bridge"}
        start = time.time()
        ok = err = total_in = total_out = 0
        frames, live = [], []
        for sym in symbols:
            df = self.store.read_output(sym)
            if df is None or df.empty:
                err += 1
                print(f"  {sym}: skipped (No interpolated data)")
                continue
            frames.append(df.sort_values("date").reset_index(drop=True)); live.append(sym)
        if frames:
            def col(df, name):
                return pd.to_numeric(df[name], errors="coerce").to_numpy(np.float64) if name in df.columns else np.full(len(df), np.nan)
            base, vol = [], []
            for df in frames:
                u, m, i = col(df, "underlying_price"), col(df, "mark_price"), col(df, "index_price")
                base.append(np.where(u != 0, u, np.where(m != 0, m, i)))
                vol.append(col(df, "volume"))
            off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
            if self._bridge_backend is None:
                from iv_interpolation_amd.bridge import HipBridgeBackend
                self._bridge_backend = HipBridgeBackend()
            out, valid, self._rng_pos, self._rng_tail = self._bridge_backend.bridge_candles(
                np.concatenate(base), np.concatenate(vol), off, PIPELINE_INLINE, self.seed, self._rng_pos, self._rng_tail,
                0.002, 1.5)
            for k, (sym, df) in enumerate(zip(live, frames)):
                a, b = int(off[k]), int(off[k + 1])
                keep = np.flatnonzero(valid[a:b])
                if len(keep) == 0:
                    err += 1
                    print(f"  {sym}: OHLCV generation failed")
                    continue
                o = out[:, a:b][:, keep]
                cand = pd.DataFrame({"symbol": df["symbol"].to_numpy()[keep], "timestamp": df["date"].to_numpy()[keep],
                                     "open": o[0], "high": o[1], "low": o[2], "close": o[3], "volume": o[4],
                                     "source_price": o[5], "is_synthetic": True})
                self.store.write_table(MINUTE_TABLE, sym, cand)
                ok += 1; total_in += len(df); total_out += len(cand)
                print(f"  {sym}: {len(df)} -> {len(cand)} candles")
        duration = time.time() - start
        print(f"\nDATA BRIDGE COMPLETE: {duration:.1f}s, success {ok}, errors {err}, OHLCV candles {total_out:,}")
        return {"success": ok > 0, "symbols_processed": ok, "total_input": total_in, "total_output": total_out,
                "duration": duration}

    def run_task2_candle_reconstruction(self, symbols: List[str] = None, batch_id: int = None) -> dict:
        """Reference :567-710: 1-minute -> 5-minute candles (first / max / min / last / sum, groups of fewer than five
        rows dropped), all symbols in one launch."""
        from iv_interpolation_amd.candles import CandleReconstructor
        print("\nTASK 2: CANDLE RECONSTRUCTION (MI355X engine)")
        print("-" * 40)
        if symbols is None:                                                   # anti-join of :623-639
            done = set(self.store.symbols(CANDLE_TABLE))
            symbols = [s for s in self.store.symbols(MINUTE_TABLE) if s not in done]
        if not symbols:
            return {"success": False, "error": "No symbols found for Task 2"}
        if batch_id is None:
            batch_id = int(time.time())
        start = time.time()
        ok = err = total_in = total_out = 0
        frames, live = [], []
        for sym in symbols:
            df = self.store.read_table(MINUTE_TABLE, sym)
            if df is None or df.empty:
                err += 1; print(f"  {sym}: skipped (No minute candles found)"); continue
            if len(df) < 5:
                err += 1; print(f"  {sym}: skipped (Insufficient data for 5-min candles)"); continue
            frames.append(df[["symbol", "timestamp", "open", "high", "low", "close", "volume"]]); live.append(sym)
        if frames:
            rec = CandleReconstructor("5min", backend=self._candle_backend)
            for sym, src, res in zip(live, frames, rec.reconstruct_batch(frames)):
                if res is None or res.empty:
                    err += 1; print(f"  {sym}: Reconstruction failed"); continue
                res = res[["timestamp", "open", "high", "low", "close", "volume", "symbol"]].copy()     # :689-704 column order
                res["frequency"] = "5min"; res["source_candles"] = 5; res["batch_id"] = batch_id          # :663-666
                self.store.write_table(CANDLE_TABLE, sym, res)
                ok += 1; total_in += len(src); total_out += len(res)
                print(f"  {sym}: {len(src)} -> {len(res)} candles ({len(src) / len(res):.1f}:1)")
        duration = time.time() - start
        print(f"\nTASK 2 COMPLETE: {duration:.1f}s, success {ok}, errors {err}, 5-min candles {total_out:,}")
        return {"success": ok > 0, "batch_id": batch_id, "symbols_processed": ok, "total_input": total_in,
                "total_output": total_out, "duration": duration}

    def _interpolated_frames(self) -> list:
        """The non-empty frames of interpolated_trading_tickers, in symbol order (input of the surface and smile tasks)."""
        symbols = self.store.symbols("interpolated_trading_tickers")
        return [f for f in (self.store.read_output(s) for s in symbols) if f is not None and not f.empty]

    def run_surfaces(self) -> dict:
        """Per-minute IV surface snapshots: every symbol of interpolated_trading_tickers is pivoted
        into one (expiry x strike) grid per underlying and minute, each grid goes through the surface engine, and one
        `iv_surfaces` table per underlying is written (columns underlying, date, spot, tenor, moneyness, iv, status)."""
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder
        print("\nSURFACES: PER-MINUTE IV SURFACE SNAPSHOTS (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for surfaces"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_snap = 0
        for res in results:
            table = builder.to_frame([res])
            self.store.write_table(SURFACE_TABLE, res.underlying, table)
            n = int(table["date"].nunique())
            n_snap += n
            print(f"  {res.underlying}: {len(res.expiries)} expiries x {len(res.strikes)} strikes, {n} snapshots")
        skipped = results[0].skipped_symbols if results else 0
        duration = time.time() - start
        print(f"\nSURFACES COMPLETE: {duration:.1f}s, underlyings {len(results)}, snapshots {n_snap:,}, skipped symbols {skipped}")
        return {"success": n_snap > 0, "underlyings": len(results), "snapshots": n_snap, "skipped_symbols": skipped,
                "duration": duration}

    def run_smiles(self) -> dict:
        """Delta-quoted smile summary: the snapshots of run_surfaces, then the ATM / 25-delta /
        10-delta points of every tenor on the device, and one `iv_smiles` table per underlying (rule D7: columns
        underlying, date, spot, tenor, atm, rr_10, bf_10, rr_25, bf_25)."""
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, smile_summary
        print("\nSMILES: DELTA-QUOTED SMILE POINTS (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for smiles"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = 0
        for res, q in zip(results, builder.smiles(results)):
            table = smile_summary([q], [res])
            self.store.write_table(SMILE_TABLE, res.underlying, table)
            n_rows += len(table)
            print(f"  {res.underlying}: {int(table['date'].nunique())} snapshots x {len(res.tenors)} tenors")
        duration = time.time() - start
        print(f"\nSMILES COMPLETE: {duration:.1f}s, underlyings {len(results)}, rows {n_rows:,}")
        return {"success": n_rows > 0, "underlyings": len(results), "rows": n_rows, "duration": duration}

    def run_arbitrage(self) -> dict:
        """Static-arbitrage report: the snapshots of run_surfaces, then the calendar / butterfly
        check of every node on the device, and one `iv_arbitrage` table per underlying (rule A8: columns underlying, date,
        spot, evaluated, calendar, butterfly, local_vol_nodes, min_numerator, min_density_factor, arbitrage_free)."""
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, arbitrage_frame
        print("\nARBITRAGE: STATIC-ARBITRAGE REPORT (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the arbitrage report"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_free = 0
        for res, rep in zip(results, builder.arbitrage(results)):
            table = arbitrage_frame([rep], [res])
            self.store.write_table(ARBITRAGE_TABLE, res.underlying, table)
            n_rows += len(table)
            free = int(table["arbitrage_free"].sum())
            n_free += free
            print(f"  {res.underlying}: {len(table)} snapshots, {free} arbitrage-free")
        duration = time.time() - start
        print(f"\nARBITRAGE COMPLETE: {duration:.1f}s, underlyings {len(results)}, rows {n_rows:,}, arbitrage-free {n_free:,}")
        return {"success": n_rows > 0, "underlyings": len(results), "rows": n_rows, "arbitrage_free_snapshots": n_free,
                "duration": duration}

    def run_volindex(self) -> dict:
        """Model-free volatility index: the snapshots of run_surfaces, then the strike integrals of
        every tenor row and the 30-day constant-maturity index on the device, and one `iv_volindex` table per underlying
        (rule M8: columns underlying, date, spot, vix_30d, flags_30d)."""
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, volindex_frame
        print("\nVOLINDEX: MODEL-FREE VOLATILITY INDEX (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the volatility index"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_idx = 0
        for res, rep in zip(results, builder.moments(results)):
            table = volindex_frame([rep], [res])
            self.store.write_table(VOLINDEX_TABLE, res.underlying, table)
            n_rows += len(table)
            finite = int(table["vix_30d"].notna().sum())
            n_idx += finite
            print(f"  {res.underlying}: {len(table)} snapshots, {finite} with a 30-day index")
        duration = time.time() - start
        print(f"\nVOLINDEX COMPLETE: {duration:.1f}s, underlyings {len(results)}, rows {n_rows:,}, indexed {n_idx:,}")
        return {"success": n_rows > 0, "underlyings": len(results), "rows": n_rows, "indexed_snapshots": n_idx,
                "duration": duration}

    def run_svi(self) -> dict:
        """Raw SVI slices: the snapshots of run_surfaces, then one parametric fit per tenor row with
        its butterfly check on the device, and one `iv_svi` table per underlying (rule V9: columns underlying, date, spot,
        tenor, a, b, rho, m, sigma, rmse_vol, max_vol_err, g_min, flags)."""
        from iv_interpolation_amd import _lib
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, svi_frame
        print("\nSVI: RAW SVI SLICES WITH A BUTTERFLY CHECK (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the SVI slices"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_fit = n_bf = 0
        for res, rep in zip(results, builder.svi(results)):
            table = svi_frame([rep], [res])
            self.store.write_table(SVI_TABLE, res.underlying, table)
            n_rows += len(table)
            fl = table["flags"].to_numpy()
            fitted, bf = int(((fl & _lib.SV_DEAD) == 0).sum()), int(((fl & _lib.SV_BUTTERFLY) != 0).sum())
            n_fit += fitted
            n_bf += bf
            print(f"  {res.underlying}: {len(table)} rows, {fitted} fitted, {bf} with butterfly arbitrage")
        duration = time.time() - start
        print(f"\nSVI COMPLETE: {duration:.1f}s, underlyings {len(results)}, rows {n_rows:,}, fitted {n_fit:,}, butterfly {n_bf:,}")
        return {"success": n_rows > 0, "underlyings": len(results), "rows": n_rows, "fitted_rows": n_fit, "butterfly_rows": n_bf,
                "duration": duration}

    @staticmethod
    def _book(frames, book_file: Optional[str]):
        """The book of run_risk and run_explain: every listed contract of the chain with quantity +1, or the CSV `book_file`
        (symbol, quantity) joined to it.  Returns (book, None) or (None, what is wrong with the file)."""
        from iv_interpolation_amd.snapshots import listed_book
        book = listed_book(frames)
        if book_file:
            held = pd.read_csv(book_file)
            for c in ("symbol", "quantity"):
                if c not in held.columns:
                    return None, f"{book_file}: no column {c!r}"
            held = held.assign(symbol=held["symbol"].astype(str), quantity=pd.to_numeric(held["quantity"], errors="coerce"))
            unknown = sorted(set(held["symbol"]) - set(book["symbol"]))
            if unknown:
                return None, f"{book_file}: not listed in the chain: {unknown[:4]}"
            twice = sorted(set(held["symbol"][held["symbol"].duplicated()]))
            if twice:
                return None, f"{book_file}: listed more than once: {twice[:4]}"
            bad = held["symbol"][~np.isfinite(held["quantity"].to_numpy(np.float64))].tolist()
            if bad:
                return None, f"{book_file}: the quantity is not a finite number: {bad[:4]}"
            book = book.drop(columns="quantity").merge(held[["symbol", "quantity"]], on="symbol", how="inner")
        return book, None

    def run_risk(self, book_file: Optional[str] = None) -> dict:
        """Book risk: the snapshots of run_surfaces and the slices of run_svi, then the smile-aware
        Greeks of a book of options, its net Greeks and its scenario P&L grid per snapshot on the device.  The book is every
        listed contract of the chain (rule S1) with quantity +1, or the CSV `book_file` with the columns symbol, quantity
        (symbols of the chain; one not listed, one listed twice or a quantity that is not a finite number is an error; an
        underlying without an option of the book gets no tables).  One `iv_risk` table (columns underlying, date, spot, price,
        delta_ss, delta_sm, gamma_ss, gamma_sm, vega, theta, gross, n_dead) and one `iv_scenarios` table (columns underlying,
        date, spot, spot_shock, vol_shock, dynamic, pnl, flags) per underlying."""
        from iv_interpolation_amd import _lib
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, risk_frame, scenario_frame
        print("\nRISK: SMILE-AWARE GREEKS AND SCENARIO P&L OF A BOOK (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the book risk"}
        start = time.time()
        book, error = self._book(frames, book_file)
        if error:
            return {"success": False, "error": error}
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_fit = n_bf = n_risk = n_scen = n_dead = 0
        for res, fit in zip(results, builder.svi(results)):
            sv = _host_flags(fit.flags)[_host_flags(res.quotes) > 0]
            n_rows += sv.size
            n_fit += int(((sv & _lib.SV_DEAD) == 0).sum())
            n_bf += int(((sv & _lib.SV_BUTTERFLY) != 0).sum())
            held = book[book["underlying"] == res.underlying].reset_index(drop=True)
            if held.empty:                                   # no position in this underlying: no tables for it
                print(f"  {res.underlying}: no option of the book, skipped")
                continue
            rep = builder.risk([res], held, [fit])
            table, scen = risk_frame(rep, [res]), scenario_frame(rep, [res])
            self.store.write_table(RISK_TABLE, res.underlying, table)
            self.store.write_table(SCENARIO_TABLE, res.underlying, scen)
            dead = int(table["n_dead"].sum())
            n_risk += len(table)
            n_scen += len(scen)
            n_dead += dead
            print(f"  {res.underlying}: {len(held)} options, {len(table)} snapshots, {len(scen)} scenario rows, {dead} dead option marks")
        duration = time.time() - start
        print(f"\nRISK COMPLETE: {duration:.1f}s, underlyings {len(results)}, snapshots {n_risk:,}, scenario rows {n_scen:,}, dead {n_dead:,}")
        return {"success": n_risk > 0, "underlyings": len(results), "rows": n_rows, "fitted_rows": n_fit, "butterfly_rows": n_bf,
                "risk_rows": n_risk, "scenario_rows": n_scen, "dead_options": n_dead, "duration": duration}

    def run_explain(self, book_file: Optional[str] = None, lag: int = 1) -> dict:
        """P&L explain: the snapshots of run_surfaces and the slices of run_svi, then the P&L of a book
        of options between every snapshot and the one `lag` snapshots later, split into theta, delta, gamma, vega and a
        remainder under sticky strike and under sticky moneyness, on the device.  The book is run_risk's.  One `iv_explain`
        table per underlying (columns underlying, start, end, dS, actual, theta_pnl, delta_ss, gamma_ss, vega_ss, resid_ss,
        delta_sm, gamma_sm, vega_sm, resid_sm, value, gross, n_dead).  Besides run_svi's keys the result has explain_rows,
        dead_options and, per dynamic, unexplained_ss / unexplained_sm: the sum of |net remainder| over the sum of |net actual|
        over the pairs with a finite net (NaN without one): the dynamic with the smaller figure explains the chain better."""
        from iv_interpolation_amd import _lib
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, explain_frame
        print("\nEXPLAIN: P&L OF A BOOK BETWEEN SNAPSHOTS UNDER BOTH SMILE DYNAMICS (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the P&L explain"}
        if int(lag) != lag or lag < 1:
            return {"success": False, "error": f"lag {lag!r} is not an integer >= 1"}
        start = time.time()
        book, error = self._book(frames, book_file)
        if error:
            return {"success": False, "error": error}
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_fit = n_bf = n_pairs = n_dead = 0
        s_actual = s_ss = s_sm = 0.0
        for res, fit in zip(results, builder.svi(results)):
            sv = _host_flags(fit.flags)[_host_flags(res.quotes) > 0]
            n_rows += sv.size
            n_fit += int(((sv & _lib.SV_DEAD) == 0).sum())
            n_bf += int(((sv & _lib.SV_BUTTERFLY) != 0).sum())
            held = book[book["underlying"] == res.underlying].reset_index(drop=True)
            if held.empty:                                   # no position in this underlying: no table for it
                print(f"  {res.underlying}: no option of the book, skipped")
                continue
            table = explain_frame(builder.explain([res], held, [fit], lag=int(lag)), [res])
            self.store.write_table(EXPLAIN_TABLE, res.underlying, table)
            live = table[np.isfinite(table["actual"].to_numpy(np.float64))]
            s_actual += float(live["actual"].abs().sum())
            s_ss += float(live["resid_ss"].abs().sum())
            s_sm += float(live["resid_sm"].abs().sum())
            dead = int(table["n_dead"].sum())
            n_pairs += len(table)
            n_dead += dead
            print(f"  {res.underlying}: {len(held)} options, {len(table)} pairs, {dead} dead option marks")
        duration = time.time() - start
        un_ss, un_sm = (s_ss / s_actual, s_sm / s_actual) if s_actual > 0 else (float("nan"), float("nan"))
        print(f"\nEXPLAIN COMPLETE: {duration:.1f}s, underlyings {len(results)}, pairs {n_pairs:,}, dead {n_dead:,}, "
              f"unexplained: sticky strike {un_ss:.3%}, sticky moneyness {un_sm:.3%}")
        return {"success": n_pairs > 0, "underlyings": len(results), "rows": n_rows, "fitted_rows": n_fit, "butterfly_rows": n_bf,
                "explain_rows": n_pairs, "dead_options": n_dead, "unexplained_ss": un_ss, "unexplained_sm": un_sm, "duration": duration}

    def run_var(self, book_file: Optional[str] = None, lag: int = 1, window: int = 256, levels=(0.05, 0.01), min_scenarios: int = 20) -> dict:
        """Historical-simulation VaR and expected shortfall: the snapshots of run_surfaces and the slices
        of run_svi, then, per snapshot, the book revalued on the surface under each of the last `window` moves the chain made
        over `lag` snapshots, and the tail of that P&L distribution at the tail probabilities `levels`, on the device (NaN for a
        snapshot with fewer than `min_scenarios` valid scenarios).  The book
        is run_risk's.  One `iv_var` table per underlying (var_frame's columns).  Besides run_svi's keys the result has var_rows,
        dead_options and `backtest`: per level a dict(tp, eligible, exceedances, exceedance_rate): eligible = the snapshots with a
        finite VaR whose pair p -> p + lag has a finite net actual P&L in the P&L explain, exceedances = those whose actual P&L is
        below -VaR, exceedance_rate = their share (NaN without an eligible snapshot), to be read beside tp."""
        return self._var_stage(book_file, lag, window, levels, min_scenarios)

    def _var_stage(self, book_file, lag, window, levels, min_scenarios, each=None, scored=None) -> dict:
        """The stage behind run_var and run_varattrib: run_var's work and result; each(builder, res, held, fit, reports), when
        given, is called once per underlying with the VarReports just made, after its iv_var table is written; scored(res, both),
        when given, once per underlying with the rows of the back-test: iv_var's columns beside `actual`."""
        from iv_interpolation_amd import _lib
        from iv_interpolation_amd.engine import hsim_settings
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, explain_frame, var_frame
        print("\nVAR: HISTORICAL-SIMULATION VAR AND EXPECTED SHORTFALL OF A BOOK (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the VaR"}
        try:
            lag, window, levels, min_scenarios, _ = hsim_settings(lag, window, levels, min_scenarios)
        except (ValueError, TypeError) as e:
            return {"success": False, "error": str(e)}
        start = time.time()
        book, error = self._book(frames, book_file)
        if error:
            return {"success": False, "error": error}
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_fit = n_bf = n_var = n_dead = 0
        eligible, exceed = [0] * len(levels), [0] * len(levels)
        for res, fit in zip(results, builder.svi(results)):
            sv = _host_flags(fit.flags)[_host_flags(res.quotes) > 0]
            n_rows += sv.size
            n_fit += int(((sv & _lib.SV_DEAD) == 0).sum())
            n_bf += int(((sv & _lib.SV_BUTTERFLY) != 0).sum())
            held = book[book["underlying"] == res.underlying].reset_index(drop=True)
            if held.empty:                                   # no position in this underlying: no table for it
                print(f"  {res.underlying}: no option of the book, skipped")
                continue
            reports = builder.var([res], held, [fit], lag=lag, window=window, tail_probs=levels, min_scenarios=min_scenarios)
            table = var_frame(reports, [res])
            self.store.write_table(VAR_TABLE, res.underlying, table)
            if each is not None:
                each(builder, res, held, fit, reports)
            realised = explain_frame(builder.explain([res], held, [fit], lag=lag), [res])
            both = table.merge(realised[["start", "actual"]], left_on="date", right_on="start", how="inner")
            actual = both["actual"].to_numpy(np.float64)
            if scored is not None:
                scored(res, both)
            for n, tp in enumerate(levels):
                var = both[f"var_{tp:g}"].to_numpy(np.float64)
                ok = np.isfinite(var) & np.isfinite(actual)
                eligible[n] += int(ok.sum())
                exceed[n] += int((ok & (actual < -var)).sum())
            dead = int(table["n_dead"].sum())
            n_var += len(table)
            n_dead += dead
            print(f"  {res.underlying}: {len(held)} options, {len(table)} snapshots, {dead} dead option marks")
        duration = time.time() - start
        backtest = [{"tp": tp, "eligible": e, "exceedances": x, "exceedance_rate": x / e if e else float("nan")}
                    for tp, e, x in zip(levels, eligible, exceed)]
        print(f"\nVAR COMPLETE: {duration:.1f}s, underlyings {len(results)}, snapshots {n_var:,}, dead {n_dead:,}, back-test: "
              + ", ".join(f"tp {b['tp']:g}: {b['exceedances']}/{b['eligible']} ({b['exceedance_rate']:.3%})" for b in backtest))
        return {"success": n_var > 0, "underlyings": len(results), "rows": n_rows, "fitted_rows": n_fit, "butterfly_rows": n_bf,
                "var_rows": n_var, "dead_options": n_dead, "backtest": backtest, "duration": duration}

    def run_varattrib(self, book_file: Optional[str] = None, lag: int = 1, window: int = 256, levels=(0.05, 0.01), min_scenarios: int = 20,
                      group_by: str = "expiry") -> dict:
        """VaR attribution: run_var, then the VaR and expected shortfall of every snapshot attributed to
        the options of the book and to groups of them (group_by: "expiry" or "side") on the device: component ES = the mean of
        the option's own P&L over the scenarios of the book's tail, component VaR = its P&L in the VaR scenario.  No level's tail
        may exceed 64 scenarios (window x level <= 64).  One `iv_var_attrib` table per underlying (var_attribution_frame's
        columns) besides run_var's `iv_var`.  The result has run_var's keys plus attrib_rows and top_contributors: the ten
        options with the largest mean |component ES / ES| at the first level over the snapshots, as a list of dicts (underlying,
        symbol, strike, expiry, callput, quantity, group, mean_abs_share, mean_ces)."""
        from iv_interpolation_amd.engine import attrib_settings
        from iv_interpolation_amd.snapshots import top_contributors, var_attribution_frame
        if group_by not in ("expiry", "side"):
            return {"success": False, "error": f"group_by {group_by!r} is neither 'expiry' nor 'side'"}
        try:
            attrib_settings(lag, window, levels, min_scenarios)
        except (ValueError, TypeError) as e:
            return {"success": False, "error": str(e)}
        rows, tops = [0], []

        def attribute(builder, res, held, fit, reports):
            rep = builder.var_attribution([res], held, reports, [fit], lag=lag, window=window, tail_probs=levels,
                                          min_scenarios=min_scenarios, group_by=group_by)
            table = var_attribution_frame(rep, [res])
            self.store.write_table(VAR_ATTRIB_TABLE, res.underlying, table)
            rows[0] += len(table)
            top = top_contributors(rep, [res])
            if "symbol" in held.columns:
                top.insert(1, "symbol", held["symbol"].to_numpy(object)[top["option"].to_numpy(np.int64)])
            tops.append(top.drop(columns="option"))
            print(f"  {res.underlying}: {len(table)} attribution rows in {len(rep[0].labels)} groups")
        result = self._var_stage(book_file, lag, window, levels, min_scenarios, each=attribute)
        if "error" in result:
            return result
        top = pd.concat(tops, ignore_index=True) if tops else pd.DataFrame()
        if len(top):
            top = top.sort_values("mean_abs_share", ascending=False, kind="stable").head(10)
            top["expiry"] = top["expiry"].astype(str)
        print(f"VAR ATTRIBUTION COMPLETE: {rows[0]:,} rows; largest mean |ES share|: "
              + ", ".join(f"{t.get('symbol', t['strike'])} {t['mean_abs_share']:.1%}" for t in top.head(3).to_dict("records")))
        return {**result, "success": result["success"] and rows[0] > 0, "attrib_rows": rows[0], "top_contributors": top.to_dict("records")}

    def run_hedge(self, book_file: Optional[str] = None, hedge_file: Optional[str] = None, rounds: int = 4, lag: int = 1, window: int = 256,
                  levels=(0.05, 0.01), min_scenarios: int = 20) -> dict:
        """Minimum-variance hedge: run_var, then per snapshot the instruments and sizes that remove the most of
        the variance of the book's scenario P&L in at most `rounds` steps, and the VaR and ES of the hedged book, on the device.
        The candidates are the CSV `hedge_file` (symbol; the word `underlying` names the underlying itself, every other symbol a
        listed contract; at most 64 per underlying) or, without one, the underlying and up to 63 listed calls nearest the money
        (snapshots.default_instruments).  One `iv_hedge` table per underlying (hedge_frame's columns) besides run_var's `iv_var`.  The
        result has run_var's keys plus hedge_rows and median_left: the median share of the row's sum of squares left after the last
        round over the snapshots with a hedge."""
        from iv_interpolation_amd.engine import hedge_settings
        from iv_interpolation_amd.snapshots import hedge_frame
        try:
            hedge_settings(lag, window, levels, min_scenarios, 1, rounds, 0)
        except (ValueError, TypeError) as e:
            return {"success": False, "error": str(e)}
        candidates, error = self._candidates(hedge_file, "the hedge")
        if error:
            return {"success": False, "error": error}
        rows, lefts, errors = [0], [], []

        def hedge(builder, res, held, fit, reports):
            inst = candidates(res, errors)
            if inst is None:
                return
            rep = builder.hedge([res], held, inst, reports, [fit], lag=lag, window=window, tail_probs=levels, min_scenarios=min_scenarios,
                                rounds=rounds)
            table = hedge_frame(rep, [res])
            self.store.write_table(HEDGE_TABLE, res.underlying, table)
            rows[0] += len(table)
            if len(table):
                lefts.extend(table.groupby("date", sort=False)["left"].last().tolist())
            print(f"  {res.underlying}: {len(table)} hedge rows over {len(rep[0].labels)} instruments")
        result = self._var_stage(book_file, lag, window, levels, min_scenarios, each=hedge)
        if "error" in result:
            return result
        if errors:
            return {"success": False, "error": errors[0]}
        left = float(np.nanmedian(lefts)) if lefts else float("nan")
        print(f"HEDGE COMPLETE: {rows[0]:,} rows; median share of the scenario variance left: {left:.3%}")
        return {**result, "success": result["success"] and rows[0] > 0, "hedge_rows": rows[0], "median_left": left}

    def _candidates(self, file: Optional[str], what: str):
        """The candidate instruments of run_hedge and run_whatif: (a function (res, errors) -> the frame of one underlying's
        candidates, or None with a message appended to errors; an error message or None).  They are the CSV `file` (symbol; the word
        `underlying` names the underlying itself, every other symbol a listed contract; at most 64 per underlying) or, without one,
        the underlying and up to 63 listed calls nearest the money (snapshots.default_instruments)."""
        from iv_interpolation_amd.snapshots import default_instruments, listed_book
        wanted = None
        frames = self._interpolated_frames()
        if not frames:
            return None, f"No interpolated data found for {what}"
        listed = listed_book(frames).set_index("symbol", drop=False)      # the candidates come from the chain, not from the book held
        if file:
            wanted = pd.read_csv(file)
            if "symbol" not in wanted.columns:
                return None, f"{file}: no column 'symbol'"
            wanted = wanted["symbol"].astype(str).tolist()
            unknown = [s for s in wanted if s.lower() != "underlying" and s not in listed.index]
            if unknown:
                return None, f"{file}: not listed in the chain: {unknown[:4]}"

        def candidates(res, errors):
            if wanted is None:                               # the underlying and the 63 listed calls nearest the money
                spots = np.asarray(_host_flags(res.spot), np.float64)
                return default_instruments(listed[listed["underlying"] == res.underlying].reset_index(drop=True),
                                           float(np.nanmedian(spots)) if np.isfinite(spots).any() else float("nan"))
            und = [s.lower() == "underlying" for s in wanted]     # the underlying and this underlying's contracts, in the file's order
            mine = [(s, u) for s, u in zip(wanted, und) if u or listed.loc[s, "underlying"] == res.underlying]
            inst = pd.DataFrame({"symbol": [s for s, _ in mine], "strike": [np.nan if u else listed.loc[s, "strike"] for s, u in mine],
                                 "expiry": [pd.NaT if u else listed.loc[s, "expiry"] for s, u in mine],
                                 "callput": ["underlying" if u else listed.loc[s, "callput"] for s, u in mine]})
            if not 1 <= len(inst) <= 64:
                errors.append(f"{file}: {len(inst)} instruments for {res.underlying}: 1 to 64 are supported")
                return None
            return inst
        return candidates, None

    def run_whatif(self, book_file: Optional[str] = None, trades_file: Optional[str] = None, sizes=(0.25, 0.5, 0.75, 1.0, 1.25, 1.5, 2.0, 3.0),
                   size_unit: str = "solo", top: int = 5, lag: int = 1, window: int = 256, levels=(0.05, 0.01), min_scenarios: int = 20) -> dict:
        """What-if VaR and ES: run_var, then per snapshot what the VaR and the expected shortfall become when a
        candidate trade is added to the book at every size of a ladder, on the device.  The candidates are the CSV `trades_file` or
        the defaults, as for run_hedge; sizes: at most 16 rungs, multiples of every candidate's own minimum-variance size
        (size_unit "solo") or quantities ("abs").  One `iv_whatif` table per underlying (whatif_frame's columns: the `top` trades per
        snapshot by ES reduction at the first level) besides run_var's `iv_var`.  The result has run_var's keys plus whatif_rows and
        median_es_reduction: the median over the snapshots of the best trade's ES reduction as a share of the book's ES."""
        from iv_interpolation_amd.engine import whatif_settings
        from iv_interpolation_amd.snapshots import whatif_frame
        try:
            sizes = [float(x) for x in sizes]
            whatif_settings(lag, window, levels, min_scenarios, 1, len(sizes))
            if size_unit not in ("solo", "abs"):
                raise ValueError(f"size_unit {size_unit!r} is neither 'solo' nor 'abs'")
            if int(top) != top or top < 1:
                raise ValueError(f"top {top!r} is not an integer >= 1")
        except (ValueError, TypeError) as e:
            return {"success": False, "error": str(e)}
        if not len(levels):
            return {"success": False, "error": "the what-if ladder ranks trades by ES: at least one tail probability is needed"}
        candidates, error = self._candidates(trades_file, "the what-if ladder")
        if error:
            return {"success": False, "error": error}
        rows, gains, errors = [0], [], []

        def whatif(builder, res, held, fit, reports):
            inst = candidates(res, errors)
            if inst is None:
                return
            rep = builder.whatif([res], held, inst, sizes, size_unit, reports, [fit], lag=lag, window=window, tail_probs=levels,
                                 min_scenarios=min_scenarios)
            table = whatif_frame(rep, [res], top=top)
            self.store.write_table(WHATIF_TABLE, res.underlying, table)
            rows[0] += len(table)
            if len(table):
                first = table.groupby("date", sort=False).first()
                name = f"es_{float(levels[0]):g}"
                with np.errstate(all="ignore"):
                    gains.extend((-first[name + "_change"] / first[name].abs()).tolist())
            print(f"  {res.underlying}: {len(table)} what-if rows over {len(rep[0].labels)} instruments x {len(sizes)} sizes")
        result = self._var_stage(book_file, lag, window, levels, min_scenarios, each=whatif)
        if "error" in result:
            return result
        if errors:
            return {"success": False, "error": errors[0]}
        gain = float(np.nanmedian(gains)) if gains else float("nan")
        print(f"WHAT-IF COMPLETE: {rows[0]:,} rows; median ES reduction of the best trade: {gain:.3%}")
        return {**result, "success": result["success"] and rows[0] > 0, "whatif_rows": rows[0], "median_es_reduction": gain}

    def run_varci(self, book_file: Optional[str] = None, lag: int = 1, window: int = 256, levels=(0.05, 0.01), min_scenarios: int = 20,
                  replicates: int = 512, block: Optional[int] = None, seed: int = 0, ci=(0.05, 0.95)) -> dict:
        """Bootstrap confidence of the VaR and ES: run_var, then per snapshot the standard error and an interval
        of every tail figure over `replicates` resamples of its valid scenarios, in circular blocks of `block` scenarios (None: the
        lag, the overlap of the scenarios), on the device.  ci: the probabilities of the interval's ends.  One `iv_var_ci` table per
        underlying (confidence_frame's columns) besides run_var's `iv_var`.  The result has run_var's keys plus ci_rows and
        median_rel_se: per level the median of se / VaR over the snapshots with a finite VaR."""
        from iv_interpolation_amd.engine import bootstrap_settings
        from iv_interpolation_amd.snapshots import confidence_frame
        try:
            bootstrap_settings(window, levels, min_scenarios, replicates, max(1, int(lag)) if block is None else block, seed, ci)
        except (ValueError, TypeError) as e:
            return {"success": False, "error": str(e)}
        rows, tables = [0], []

        def confidence(builder, res, held, fit, reports):
            rep = builder.var_confidence(reports, n_rep=replicates, block=block, seed=seed, ci=ci)
            table = confidence_frame(rep, [res])
            self.store.write_table(VAR_CI_TABLE, res.underlying, table)
            rows[0] += len(table)
            tables.append(table)
            print(f"  {res.underlying}: {len(table)} confidence rows, {rep[0].n_rep} replicates in blocks of {rep[0].block}")
        result = self._var_stage(book_file, lag, window, levels, min_scenarios, each=confidence)
        if "error" in result:
            return result
        rel = []
        for tp in levels:
            name = f"var_{float(tp):g}"
            var = np.concatenate([t[name].to_numpy(np.float64) for t in tables]) if tables else np.zeros(0)
            se = np.concatenate([t[name + "_se"].to_numpy(np.float64) for t in tables]) if tables else np.zeros(0)
            ok = np.isfinite(var)
            with np.errstate(all="ignore"):
                rel.append(float(np.nanmedian((se / var)[ok])) if ok.any() else float("nan"))
        print(f"VAR CONFIDENCE COMPLETE: {rows[0]:,} rows; median se / VaR: " + ", ".join(f"tp {float(tp):g}: {x:.1%}" for tp, x in zip(levels, rel)))
        return {**result, "success": result["success"] and rows[0] > 0, "ci_rows": rows[0], "median_rel_se": rel}

    def run_varw(self, book_file: Optional[str] = None, lag: int = 1, window: int = 256, levels=(0.05, 0.01), min_scenarios: int = 20,
                 decay: float = 0.99, vol_span: int = 0, vol_decay: float = 0.94, scale_cap: float = 3.0, min_returns: Optional[int] = None) -> dict:
        """Age-weighted, volatility-scaled VaR and ES: run_var, then per snapshot the tail of the same scenarios
        with the weight decay^s on the scenario of age s and, with vol_span > 0, every scenario scaled by the running vol of the spot
        today over that at its start (the root of the vol_decay-weighted mean of vol_span squared returns, NaN before min_returns
        of them, None: min(20, vol_span); the factor inside [1 / scale_cap, scale_cap]), on the device.  One `iv_var_w` table per underlying
        (weighted_var_frame's columns) besides run_var's `iv_var`.  The result has run_var's keys plus w_rows, backtest_w (run_var's
        back-test on the weighted VaR) and kupiec: per level dict(tp, plain, weighted) with Kupiec's likelihood ratio of the two
        back-tests (kupiec_lr), to be read against chi-squared with one degree of freedom (3.84 at 5 %)."""
        from iv_interpolation_amd.engine import age_weights, hsim_settings, weighted_settings
        from iv_interpolation_amd.snapshots import weighted_var_frame
        if min_returns is None:
            min_returns = min(20, vol_span) if isinstance(vol_span, int) and vol_span > 0 else 20
        try:
            weighted_settings(window, lag, levels, min_scenarios, vol_span, min_returns, scale_cap)
            age_weights(1, decay)
            age_weights(1, vol_decay)
            levels = hsim_settings(lag, window, levels, min_scenarios)[2]
        except (ValueError, TypeError) as e:
            return {"success": False, "error": str(e)}
        rows, tables = [0], {}
        eligible, exceed = [0] * len(levels), [0] * len(levels)

        def weigh(builder, res, held, fit, reports):
            rep = builder.var_weighted([res], reports, decay=decay, vol_span=vol_span, vol_decay=vol_decay, min_returns=min_returns, scale_cap=scale_cap)
            table = weighted_var_frame(rep, [res])
            self.store.write_table(VAR_W_TABLE, res.underlying, table)
            rows[0] += len(table)
            tables[res.underlying] = table
            print(f"  {res.underlying}: {len(table)} weighted rows, decay {decay:g}, vol span {vol_span}")

        def score(res, both):                                # run_var's eligibility and exceedance rule on varw
            names = [f"varw_{tp:g}" for tp in levels]
            mine = both[["date", "actual"]].merge(tables[res.underlying][["date"] + names], on="date", how="inner")
            actual = mine["actual"].to_numpy(np.float64)
            for n, name in enumerate(names):
                var = mine[name].to_numpy(np.float64)
                ok = np.isfinite(var) & np.isfinite(actual)
                eligible[n] += int(ok.sum())
                exceed[n] += int((ok & (actual < -var)).sum())
        result = self._var_stage(book_file, lag, window, levels, min_scenarios, each=weigh, scored=score)
        if "error" in result:
            return result
        backtest_w = [{"tp": tp, "eligible": e, "exceedances": x, "exceedance_rate": x / e if e else float("nan")}
                      for tp, e, x in zip(levels, eligible, exceed)]
        kupiec = [{"tp": b["tp"], "plain": kupiec_lr(b["eligible"], b["exceedances"], b["tp"]), "weighted": kupiec_lr(w["eligible"], w["exceedances"], w["tp"])}
                  for b, w in zip(result["backtest"], backtest_w)]
        print(f"WEIGHTED VAR COMPLETE: {rows[0]:,} rows; back-test: "
              + ", ".join(f"tp {w['tp']:g}: {w['exceedances']}/{w['eligible']} ({w['exceedance_rate']:.3%}), Kupiec LR plain {k['plain']:.2f} / weighted {k['weighted']:.2f}"
                          for w, k in zip(backtest_w, kupiec)))
        return {**result, "success": result["success"] and rows[0] > 0, "w_rows": rows[0], "backtest_w": backtest_w, "kupiec": kupiec}

    def run_distribution(self) -> dict:
        """Risk-neutral distribution: the snapshots of run_surfaces and the slices of run_svi, then the
        quantiles, level probabilities and tails of every tenor row on the device, and one `iv_distribution` table per
        underlying (rule P9: columns underlying, date, spot, tenor, forward, q_1 ... q_99, below_80 ... below_120, tail_lo,
        tail_hi, flags)."""
        from iv_interpolation_amd import _lib
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, distribution_frame
        print("\nDISTRIBUTION: RISK-NEUTRAL QUANTILES AND PROBABILITIES (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the distribution"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_live = n_amb = 0
        for res, rep in zip(results, builder.distribution(results)):
            table = distribution_frame([rep], [res])
            self.store.write_table(DISTRIBUTION_TABLE, res.underlying, table)
            n_rows += len(table)
            fl = table["flags"].to_numpy()
            live, amb = int(((fl & _lib.DS_DEAD) == 0).sum()), int(((fl & _lib.DS_AMBIGUOUS) != 0).sum())
            n_live += live
            n_amb += amb
            print(f"  {res.underlying}: {len(table)} rows, {live} live, {amb} with a non-monotone CDF")
        duration = time.time() - start
        print(f"\nDISTRIBUTION COMPLETE: {duration:.1f}s, underlyings {len(results)}, rows {n_rows:,}, live {n_live:,}, ambiguous {n_amb:,}")
        return {"success": n_rows > 0, "underlyings": len(results), "rows": n_rows, "live_rows": n_live, "ambiguous_rows": n_amb,
                "duration": duration}

    def run_calendar(self) -> dict:
        """Calendar report: the snapshots of run_surfaces and the slices of run_svi, then per snapshot
        every pair of adjacent live slices compared on the device, and one `iv_calendar` table per underlying (columns
        underlying, date, spot, tenor, next_tenor, d_min, x_min, d_atm, n_cross, x_first, x_last, flags)."""
        from iv_interpolation_amd import _lib
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, calendar_frame
        print("\nCALENDAR: CALENDAR CHECK BETWEEN THE SVI SLICES (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the calendar report"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_fit = n_bf = n_cal = n_wing = 0
        for res, fit in zip(results, builder.svi(results)):
            sv = _host_flags(fit.flags)[_host_flags(res.quotes) > 0]
            n_fit += int(((sv & _lib.SV_DEAD) == 0).sum())
            n_bf += int(((sv & _lib.SV_BUTTERFLY) != 0).sum())
            table = calendar_frame(builder.calendar([res], [fit]), [res])
            self.store.write_table(CALENDAR_TABLE, res.underlying, table)
            n_rows += len(table)
            fl = table["flags"].to_numpy()
            cal = int(((fl & _lib.SC_CALENDAR) != 0).sum())
            wing = int(((fl & (_lib.SC_WING_LEFT | _lib.SC_WING_RIGHT)) != 0).sum())
            n_cal += cal
            n_wing += wing
            print(f"  {res.underlying}: {len(table)} pairs, {cal} crossing on the grid, {wing} crossing in a wing")
        duration = time.time() - start
        print(f"\nCALENDAR COMPLETE: {duration:.1f}s, underlyings {len(results)}, pairs {n_rows:,}, calendar {n_cal:,}, wing {n_wing:,}")
        return {"success": n_rows > 0, "underlyings": len(results), "rows": n_rows, "fitted_rows": n_fit, "butterfly_rows": n_bf,
                "calendar_pairs": n_cal, "wing_pairs": n_wing, "duration": duration}

    def run_ssvi(self) -> dict:
        """Arbitrage-free SSVI surfaces: the snapshots of run_surfaces and the slices of run_svi, then one
        (rho, eta, gamma) per snapshot fitted jointly across its tenors on the device, and one `iv_ssvi` table per underlying
        (one row per live slice: columns underlying, date, spot, tenor, theta, a, b, rho, m, sigma, rmse_vol, max_vol_err,
        g_min, flags, and the snapshot's eta, gamma, rmse, sflags).  Returns run_svi's keys plus ssvi_surfaces, raised_rows."""
        from iv_interpolation_amd import _lib
        from iv_interpolation_amd.snapshots import SnapshotSurfaceBuilder, ssvi_frame, ssvi_slices_frame
        print("\nSSVI: ARBITRAGE-FREE SURFACE PER SNAPSHOT (MI355X engine)")
        print("-" * 40)
        frames = self._interpolated_frames()
        if not frames:
            return {"success": False, "error": "No interpolated data found for the SSVI surfaces"}
        start = time.time()
        builder = SnapshotSurfaceBuilder(backend=self._surface_backend)
        results = builder.build(frames)
        n_rows = n_fit = n_bf = n_surf = n_raised = 0
        for res, fit in zip(results, builder.svi(results)):
            sv = _host_flags(fit.flags)[_host_flags(res.quotes) > 0]
            n_fit += int(((sv & _lib.SV_DEAD) == 0).sum())
            n_bf += int(((sv & _lib.SV_BUTTERFLY) != 0).sum())
            rep = builder.ssvi([res], [fit])
            surf, table = ssvi_frame(rep, [res]), ssvi_slices_frame(rep, [res])
            table = table.merge(surf[["date", "eta", "gamma", "rmse", "sflags"]], on="date", how="left")
            self.store.write_table(SSVI_TABLE, res.underlying, table)
            n_rows += len(table)
            good = int(((surf["sflags"].to_numpy() & (_lib.SF_SURF_DEAD | _lib.SF_UNORDERED)) == 0).sum())
            raised = int(surf["raised_rows"].sum())
            n_surf += good
            n_raised += raised
            print(f"  {res.underlying}: {len(surf)} snapshots, {good} surfaces, {len(table)} slices, {raised} raised")
        duration = time.time() - start
        print(f"\nSSVI COMPLETE: {duration:.1f}s, underlyings {len(results)}, rows {n_rows:,}, surfaces {n_surf:,}, raised {n_raised:,}")
        return {"success": n_rows > 0, "underlyings": len(results), "rows": n_rows, "fitted_rows": n_fit, "butterfly_rows": n_bf,
                "ssvi_surfaces": n_surf, "raised_rows": n_raised, "duration": duration}

    def run_implied(self) -> dict:
        """Vol implied by the stored mark: every row of interpolated_trading_tickers that carries a
        mark_price goes through the price -> vol solver in price_mode "underlying" (mark_price is quoted in units of the
        underlying) with the row's own interest_rate, time_to_maturity, strike, callput and underlying_price, all rows of an
        underlying in one launch, and one `iv_implied` table per underlying is written (columns symbol, date, iv,
        iv_from_mark, iv_diff, flags).  The result counts the rows per flag."""
        from iv_interpolation_amd.implied import HipImpliedBackend, count_flags
        print("\nIMPLIED: VOL IMPLIED BY THE STORED MARK (MI355X engine)")
        print("-" * 40)
        groups = {}
        for sym in self.store.symbols("interpolated_trading_tickers"):
            df = self.store.read_output(sym)
            if df is None or df.empty or "mark_price" not in df.columns:
                continue
            df = df[pd.to_numeric(df["mark_price"], errors="coerce").notna()]
            if df.empty:
                continue
            side = df["callput"].astype(str).str.lower().str[:1] if "callput" in df.columns else pd.Series("", index=df.index)
            side = side.where(side.isin(["c", "p"]), "p" if sym.lower().endswith("-p") else "c")     # interpolated rows may lack it
            cols = {k: pd.to_numeric(df[k], errors="coerce").to_numpy(np.float64)
                    for k in ("iv", "mark_price", "underlying_price", "strike", "time_to_maturity", "interest_rate")}
            groups.setdefault(sym.split("-")[0], []).append(pd.DataFrame(
                {"symbol": sym, "date": df["date"].to_numpy(), **cols, "is_put": (side == "p").to_numpy(np.uint8)}))
        if not groups:
            return {"success": False, "error": "No interpolated rows with a mark_price found"}
        start = time.time()
        be = self._implied_backend or HipImpliedBackend()
        flags = []
        for underlying in sorted(groups):
            g = pd.concat(groups[underlying], ignore_index=True)
            q = be.implied_vol(*[g[k].to_numpy(np.float64) for k in ("mark_price", "underlying_price", "strike", "time_to_maturity", "interest_rate")],
                               g["is_put"].to_numpy(np.uint8), price_mode=1)
            vol, fl = np.asarray(q["vol"], np.float64), np.asarray(q["flags"], np.int32)
            table = pd.DataFrame({"symbol": g["symbol"], "date": g["date"], "iv": g["iv"], "iv_from_mark": vol,
                                  "iv_diff": vol - g["iv"].to_numpy(), "flags": fl})
            self.store.write_table(IMPLIED_TABLE, underlying, table)
            flags.append(fl)
            print(f"  {underlying}: {len(table)} rows, {int(np.isfinite(vol).sum())} with a vol")
        counts = count_flags(np.concatenate(flags))
        duration = time.time() - start
        n_rows = sum(len(f) for f in flags)
        print(f"\nIMPLIED COMPLETE: {duration:.1f}s, underlyings {len(groups)}, rows {n_rows:,}, solved {counts['solved_rows']:,}")
        return {"success": n_rows > 0, "underlyings": len(groups), "rows": n_rows, **counts, "duration": duration}

    def run_complete_pipeline(self, test_mode: bool = False, symbol_limit: int = None) -> dict:
        """Reference :740-831: Task 1 -> bridge -> Task 2 over the same symbol list, stopping at the first failed stage."""
        symbols = self.store.symbols()
        if test_mode:
            symbols = symbols[:3]
        elif symbol_limit:
            symbols = symbols[:symbol_limit]
        if not symbols:
            return {"success": False, "error": "No symbols found"}
        batch_id = int(time.time())
        t0 = time.time()
        results = {}
        try:
            results["task1"] = self.run_task1_interpolation(symbols, batch_id)
            if not results["task1"]["success"]:
                return {"success": False, "error": "Task 1 failed", "results": results}
            results["bridge"] = self.run_data_bridge(symbols, batch_id)
            if not results["bridge"]["success"]:
                return {"success": False, "error": "Data bridge failed", "results": results}
            results["task2"] = self.run_task2_candle_reconstruction(symbols, batch_id)
            if not results["task2"]["success"]:
                return {"success": False, "error": "Task 2 failed", "results": results}
            return {"success": True, "batch_id": batch_id, "duration": time.time() - t0, "results": results,
                    "final_status": self.get_pipeline_status()}
        except Exception as e:
            return {"success": False, "error": str(e), "results": results}

    def cleanup(self):
        pass


def kupiec_lr(n: int, x: int, tp: float) -> float:
    """Kupiec's proportion-of-failures likelihood ratio of x exceedances among n eligible snapshots at the tail probability tp:
    -2 [(n - x) ln(1 - tp) + x ln tp - (n - x) ln(1 - x / n) - x ln(x / n)], with 0 ln 0 = 0; NaN without an eligible snapshot.
    Under a correct VaR it is chi-squared with one degree of freedom."""
    import math
    if n <= 0:
        return float("nan")

    def xlogy(a, b):
        return a * math.log(b) if a > 0 else 0.0
    return -2.0 * (xlogy(n - x, 1.0 - tp) + xlogy(x, tp) - xlogy(n - x, 1.0 - x / n) - xlogy(x, x / n))


def _host_flags(a):
    import numpy as np
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


def main(argv=None, backend=None, bridge_backend=None, candle_backend=None, seed=None, surface_backend=None, implied_backend=None):
    parser = argparse.ArgumentParser(description="Complete Optimized Pipeline (MI355X engine)")
    parser.add_argument("--task", choices=["interpolation", "implied", "bridge", "candles", "surfaces", "smiles", "arbitrage", "volindex", "svi", "distribution", "calendar", "ssvi", "risk", "explain", "var", "varattrib", "hedge", "whatif", "varci", "varw", "all"], default="all")
    parser.add_argument("--book", metavar="FILE", help="--task risk / explain / var: a CSV of symbol, quantity (default: every listed contract, +1 each)")
    parser.add_argument("--lag", type=int, default=1, metavar="N", help="--task explain / var: the pair is snapshot p and snapshot p + N (default 1)")
    parser.add_argument("--window", type=int, default=256, metavar="W", help="--task var: scenarios kept per snapshot (default 256)")
    parser.add_argument("--levels", default="0.05,0.01", metavar="P,P", help="--task var: tail probabilities (default 0.05,0.01)")
    parser.add_argument("--min-scenarios", type=int, default=20, metavar="N", help="--task var: fewer valid scenarios than N give no VaR (default 20)")
    parser.add_argument("--hedge-with", metavar="FILE", help="--task hedge: a CSV of symbol (`underlying` or a listed contract), the candidates (default: the underlying and the 63 calls nearest the money)")
    parser.add_argument("--rounds", type=int, default=4, metavar="K", help="--task hedge: at most K instruments per snapshot, 1..8 (default 4)")
    parser.add_argument("--trades", metavar="FILE", help="--task whatif: a CSV of symbol (`underlying` or a listed contract), the candidate trades (default: as --hedge-with)")
    parser.add_argument("--sizes", default="0.25,0.5,0.75,1,1.25,1.5,2,3", metavar="LIST", help="--task whatif: the ladder of sizes, at most 16 (default 0.25,...,3)")
    parser.add_argument("--size-unit", choices=["solo", "abs"], default="solo", help="--task whatif: sizes are multiples of a candidate's own minimum-variance size, or quantities (default solo)")
    parser.add_argument("--top", type=int, default=5, metavar="N", help="--task whatif: trades kept per snapshot (default 5)")
    parser.add_argument("--replicates", type=int, default=512, metavar="R", help="--task varci: bootstrap replicates per snapshot, 1..1024 (default 512)")
    parser.add_argument("--block", type=int, default=None, metavar="L", help="--task varci: scenarios per block of the circular block bootstrap (default: the lag)")
    parser.add_argument("--seed", type=int, default=0, metavar="S", help="--task varci: the seed of the resampling (default 0)")
    parser.add_argument("--ci", default="0.05,0.95", metavar="P,P", help="--task varci: the probabilities of the interval's ends (default 0.05,0.95)")
    parser.add_argument("--decay", type=float, default=0.99, metavar="D", help="--task varw: the weight of a scenario of age s is D^s, D in (0, 1] (default 0.99)")
    parser.add_argument("--vol-span", type=int, default=0, metavar="M", help="--task varw: returns per running vol of the spot, 0..1024; 0 = no volatility scaling (default 0)")
    parser.add_argument("--vol-decay", type=float, default=0.94, metavar="D", help="--task varw: the decay of the running vol's weights (default 0.94)")
    parser.add_argument("--scale-cap", type=float, default=3.0, metavar="C", help="--task varw: the scaling factor is held inside [1/C, C] (default 3)")
    parser.add_argument("--group-by", choices=["expiry", "side"], default="expiry", help="--task varattrib: the groups the VaR is attributed to (default expiry)")
    parser.add_argument("--test", action="store_true", help="Test mode with 3 symbols")
    parser.add_argument("--symbols", type=int, help="Limit number of symbols")
    parser.add_argument("--estimate", action="store_true", help="Show estimates only")
    parser.add_argument("--setup-only", action="store_true", help="Setup tables only")
    parser.add_argument("--data-dir", help="frame store directory (default: config.data_dir / $IVS_DATA_DIR)")
    parser.add_argument("--synthetic", type=int, metavar="N", help="first fill the store with N synthetic hourly symbols")
    args = parser.parse_args(argv)
    try:
        config = get_config()
        pipeline = CompleteOptimizedPipeline(config, data_dir=args.data_dir, backend=backend, bridge_backend=bridge_backend,
                                             candle_backend=candle_backend, seed=seed, surface_backend=surface_backend,
                                             implied_backend=implied_backend)
        if args.synthetic:
            for i in range(args.synthetic):
                sym = f"btc-20mar23-{20000 + 500 * i}-c"
                pipeline.store.write_source(sym, synthetic_symbol(sym, seed=i))
        if args.setup_only:
            pipeline.setup_database_tables()
            print("Setup complete")
            return 0
        if args.estimate:
            st = pipeline.get_pipeline_status()
            print(f"Source data: {st['source_rows']:,} rows, {st['source_symbols']:,} symbols")
            print(f"Task 1 progress: {st['task1_symbols']}/{st['source_symbols']} symbols")
            return 0
        if args.task == "all":
            result = pipeline.run_complete_pipeline(test_mode=args.test, symbol_limit=args.symbols)
        else:
            symbols = None
            if args.symbols or args.test:
                symbols = pipeline.store.symbols()[:3 if args.test else args.symbols]
            if args.task == "interpolation":
                result = pipeline.run_task1_interpolation(symbols)
            elif args.task == "implied":
                result = pipeline.run_implied()
            elif args.task == "bridge":
                result = pipeline.run_data_bridge(symbols)
            elif args.task == "surfaces":
                result = pipeline.run_surfaces()
            elif args.task == "smiles":
                result = pipeline.run_smiles()
            elif args.task == "arbitrage":
                result = pipeline.run_arbitrage()
            elif args.task == "volindex":
                result = pipeline.run_volindex()
            elif args.task == "svi":
                result = pipeline.run_svi()
            elif args.task == "distribution":
                result = pipeline.run_distribution()
            elif args.task == "calendar":
                result = pipeline.run_calendar()
            elif args.task == "ssvi":
                result = pipeline.run_ssvi()
            elif args.task == "risk":
                result = pipeline.run_risk(args.book)
            elif args.task == "explain":
                result = pipeline.run_explain(args.book, args.lag)
            elif args.task == "var":
                result = pipeline.run_var(args.book, args.lag, args.window, [float(x) for x in args.levels.split(",") if x.strip()], args.min_scenarios)
            elif args.task == "varattrib":
                result = pipeline.run_varattrib(args.book, args.lag, args.window, [float(x) for x in args.levels.split(",") if x.strip()],
                                                args.min_scenarios, args.group_by)
            elif args.task == "hedge":
                result = pipeline.run_hedge(args.book, args.hedge_with, args.rounds, args.lag, args.window,
                                            [float(x) for x in args.levels.split(",") if x.strip()], args.min_scenarios)
            elif args.task == "whatif":
                result = pipeline.run_whatif(args.book, args.trades, [float(x) for x in args.sizes.split(",") if x.strip()], args.size_unit, args.top,
                                             args.lag, args.window, [float(x) for x in args.levels.split(",") if x.strip()], args.min_scenarios)
            elif args.task == "varci":
                result = pipeline.run_varci(args.book, args.lag, args.window, [float(x) for x in args.levels.split(",") if x.strip()], args.min_scenarios,
                                            args.replicates, args.block, args.seed, [float(x) for x in args.ci.split(",") if x.strip()])
            elif args.task == "varw":
                result = pipeline.run_varw(args.book, args.lag, args.window, [float(x) for x in args.levels.split(",") if x.strip()], args.min_scenarios,
                                           args.decay, args.vol_span, args.vol_decay, args.scale_cap)
            else:
                result = pipeline.run_task2_candle_reconstruction(symbols)
        return 0 if result["success"] else 1
    except KeyboardInterrupt:
        print("\nPipeline interrupted by user")
        return 130


if __name__ == "__main__":
    sys.exit(main())
