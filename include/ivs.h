/*
 * ivs.h -- C ABI of the MI355X-native IV interpolation engine (libivs.so).
 *
 * This is the drop-in boundary for the reference hot path
 *   /root/reference/src/interpolation/core.py:16-85  IVInterpolator.interpolate_symbol
 * The reference has no FFI today (plain Python calling pandas); these entry points are
 * what a ctypes binding inside that class binds (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - plain C linkage, no exceptions, no torch types; every pointer is a DEVICE pointer
 *     owned by the caller (e.g. torch tensor .data_ptr()) unless marked host;
 *   - fp64, row-major, contiguous; NaN in a value array means "missing quote" (not a knot);
 *   - asynchronous on `stream` (a hipStream_t passed as void*, NULL = default stream);
 *   - no allocation, no synchronisation inside a call (safe to capture in a hipGraph): every entry point
 *     that needs device scratch takes a caller-owned `workspace` sized by its *_workspace_bytes() function;
 *   - return 0 on success or a negative IVS_E* code; ivs_last_error() gives the text
 *     (thread local).  Numerical conditions (too few knots) are reported per item in
 *     the `status` array, never through the return code.
 */
#ifndef IVS_H
#define IVS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVS_ABI_VERSION 5

/* interpolation methods: the pandas method names that core.py:61 forwards
 * (`merged[col].interpolate(method=self.method)`) and that this engine implements */
enum {
    IVS_LINEAR      = 0, /* 'linear','index','values': np.interp; NaN left of the first knot, hold-last on the right */
    IVS_CUBIC       = 1, /* 'cubic': interp1d(kind=3) = not-a-knot spline; NaN outside the hull; needs >= 4 knots */
    IVS_CUBICSPLINE = 2, /* 'cubicspline': CubicSpline(not-a-knot); 2 knots = line, 3 = parabola; NaN left, extrapolates right */
    IVS_SLINEAR     = 3, /* 'slinear': interp1d(kind=1); NaN outside the hull; needs >= 2 knots */
    IVS_NEAREST     = 4, /* 'nearest': interp1d nearest, ties to the left knot; NaN outside the hull; >= 1 knot */
    IVS_ZERO        = 5, /* 'zero': order-0 spline = left knot's value; NaN outside the hull; >= 1 knot */
    IVS_PCHIP       = 6, /* 'pchip': PchipInterpolator; NaN left, extrapolates right; >= 2 knots */
    IVS_AKIMA       = 7, /* 'akima': Akima1DInterpolator; NaN outside the hull; >= 3 knots (scipy's 2-knot case is undefined) */
    IVS_FROM_DERIVATIVES = 8, /* 'from_derivatives' / 'piecewise_polynomial': BPoly on values = Bernstein-form lines; NaN outside; >= 2 */
    IVS_QUADRATIC   = 9, /* 'quadratic': interp1d(kind=2) = make_interp_spline(k=2), knots at the midpoints of the sites; NaN outside; >= 3 */
    IVS_BARYCENTRIC = 10,/* 'barycentric': scipy barycentric_interpolate, ONE polynomial through all valid knots; NaN left of the
                            first knot, the polynomial continues on the right; 1..IVS_POLY_MAX_KNOTS knots; 1-D kernels only */
    IVS_KROGH       = 11,/* 'krogh': scipy krogh_interpolate, the same polynomial in Newton form (divided differences); 1-D only */
    IVS_PAD         = 12,/* 'pad' / 'ffill': pandas pad_or_backfill forward (core.py:61 forwards the name; pandas 2.x still runs
                            it, with a FutureWarning): the last valid knot at or before the row; NaN left of the first knot,
                            hold-last on the right; never raises (>= 0 knots) */
    IVS_BFILL       = 13 /* 'bfill' / 'backfill': the mirror -- the first valid knot at or after the row; NaN right of the last
                            knot, the first knot's value on the left */
};
#define IVS_POLY_MAX_KNOTS 32   /* above this the reference's own polynomial is numerical noise: IVS_ST_ILL_CONDITIONED */
/* surfaces: methods 0-9 run on the fast (row-pass / one-pass / masked) kernels, 12 and 13 on the generic surface kernel,
 * 10 and 11 are rejected (EINVAL); the 1-D kernels take all of 0-13 */

/* return codes */
enum {
    IVS_OK            = 0,
    IVS_EINVAL        = -22, /* bad argument (null pointer, negative size, unknown method) */
    IVS_ERANGE        = -34, /* shape outside what the kernels support (see ivs_last_error) */
    IVS_ENOMEM        = -12, /* workspace too small */
    IVS_ELAUNCH       = -5   /* HIP launch error */
};

/* per-item status bits written to `status` arrays */
enum {
    IVS_ST_OK            = 0,
    IVS_ST_TOO_FEW_KNOTS = 1, /* the reference's scipy call raises here -> interpolate_symbol returns None */
    IVS_ST_BAD_SHAPE     = 2, /* ragged surface whose k_off span is negative, exceeds nK or leaves the strike array: skipped, outputs untouched */
    IVS_ST_ILL_CONDITIONED = 4 /* 'barycentric' / 'krogh' with more than IVS_POLY_MAX_KNOTS valid knots: values are NaN */
};

int         ivs_version(void);        /* IVS_ABI_VERSION of the loaded library */
const char* ivs_last_error(void);     /* host pointer, valid until the next call on this thread */
int         ivs_device_count(void);   /* number of visible HIP devices (0 if none) */

/*
 * Batch of 1-D series, C channels sharing knot coordinates: the arithmetic of
 * core.py:58-61 (three channels of one symbol) for S symbols at once.
 *
 *   xk  [total_knots]            knot coordinates of all series back to back, ascending within a series
 *   yk  [C][yk_stride]           channel c of knot i at yk[c*yk_stride + i]; NaN = not a knot for that channel
 *   knot_off [S+1]               CSR offsets into xk / yk
 *   xq  [total_queries] or NULL  query coordinates; NULL = 0,1,..,m_s-1 per series (the reference's RangeIndex)
 *   q_off [S+1]                  CSR offsets into xq / out
 *   out [C][out_stride]          result of channel c, query i at out[c*out_stride + i]; a query that coincides with a
 *                                knot of the channel returns that knot's value (the merged column of the reference's
 *                                frame), also when status reports too few knots to interpolate between them
 *   status [S*C]                 IVS_ST_* per (series, channel)
 *   workspace                    ivs_interp1d_workspace_bytes(total_knots, S, C) bytes of device memory
 */
size_t ivs_interp1d_workspace_bytes(int64_t total_knots, int64_t n_series, int32_t n_channels);
int ivs_interp1d_batch_f64(const double* xk, const double* yk, int64_t yk_stride, const int64_t* knot_off,
                           int64_t n_series, int32_t n_channels, int64_t total_knots,
                           const double* xq, const int64_t* q_off, int64_t total_queries,
                           double* out, int64_t out_stride, int32_t* status, int32_t method,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same call with the Black-Scholes Greeks as an EPILOGUE (reference config.py:46 `preserve_greeks`: "Recalculate Greeks
 * after interpolation"; columns delta, gamma, theta, vega, rho of src/database/schema.py:36-40; formulas
 * src/interpolation/greeks.py:12-43).  The reference never wires the flag up; here the eval kernel forms the five values
 * of an output row from the channel values it has just produced (a row that is a knot of a channel uses the source cell,
 * as the reference's frame does) plus the forward-filled strike / interest_rate / callput of that row:
 *   ch_iv, ch_underlying, ch_ttm     channel numbers of sigma, S and T inside yk
 *   fill_idx [rows][fill_stride]     output of ivs_ffill_index_batch for this batch (same q_off); row_strike / row_rate /
 *                                    row_callput = its row for that column, or -1 when the frame has no such column
 *                                    (no strike: NaN Greeks; no interest_rate: 0.0, the schema default; no callput: call)
 *   strike_src, rate_src [total_src] source-row values of those columns; is_put_src: 0 call, 1 put, 2 null (-> NaN Greeks)
 *   greeks [5][greeks_stride]        delta, gamma, theta (per day), vega and rho (per 1 %), put rho unsigned like the reference
 */
int ivs_interp1d_greeks_batch_f64(const double* xk, const double* yk, int64_t yk_stride, const int64_t* knot_off,
                                  int64_t n_series, int32_t n_channels, int64_t total_knots,
                                  const double* xq, const int64_t* q_off, int64_t total_queries,
                                  double* out, int64_t out_stride, int32_t* status, int32_t method,
                                  int32_t ch_iv, int32_t ch_underlying, int32_t ch_ttm,
                                  const int32_t* fill_idx, int64_t fill_stride, int32_t row_strike, int32_t row_rate,
                                  int32_t row_callput, const double* strike_src, const double* rate_src,
                                  const uint8_t* is_put_src, double* greeks, int64_t greeks_stride,
                                  void* workspace, size_t workspace_bytes, void* stream);

/*
 * Forward-fill gather index: the "index of the last valid source row at or before
 * output row i" of core.py:64-68 (nine `fillna(method='ffill')` columns), for S symbols.
 *
 *   src_pos [total_src]          merged-frame row position of every source row, ascending within a series
 *   src_off [S+1]                CSR offsets into src_pos / valid
 *   valid   [n_cols][valid_stride]  1 = source cell is non-null in that column
 *   q_off   [S+1]                CSR offsets of the output rows (row i of series s is position i - q_off[s])
 *   idx_out [n_cols][out_stride] flat source-row index to gather from, or -1 (stays null)
 */
int ivs_ffill_index_batch(const int64_t* src_pos, const int64_t* src_off, const uint8_t* valid, int64_t valid_stride,
                          int32_t n_cols, const int64_t* q_off, int64_t n_series, int64_t total_queries,
                          int32_t* idx_out, int64_t out_stride, void* stream);

/*
 * Columnar egress of the forward-filled columns (core.py:64-68 for every symbol at once): column c of the long output
 * frame is gathered on the device with the index ivs_ffill_index_batch produced,
 *   out[c][g] = idx[idx_row[c]][g] >= 0 ? src[c][idx[idx_row[c]][g]] : missing     (missing: NaN / -1)
 * f64 for numeric columns, i32 for the codes of object columns (symbol, callput); idx_row [n_cols] (device) names the
 * row of idx each column uses.
 */
int ivs_gather_rows_f64(const double* src, int64_t src_stride, const int32_t* idx, int64_t idx_stride, const int32_t* idx_row,
                        int32_t n_cols, int64_t n, double* out, int64_t out_stride, void* stream);
int ivs_gather_rows_i32(const int32_t* src, int64_t src_stride, const int32_t* idx, int64_t idx_stride, const int32_t* idx_row,
                        int32_t n_cols, int64_t n, int32_t* out, int64_t out_stride, void* stream);

/*
 * Row bookkeeping of the long output frame on the device: date_ns[g] = first_ns[s] + (g - q_off[s]) minutes (s = the
 * symbol of row g; valid for symbols without duplicate timestamps) and keep[g] = the row survives the reference's dropna
 * (core.py:74) in a symbol that did not fail (status[s][c] != 0 on a channel with needs[s][c] -> the symbol is None).
 * chan [n_channels][chan_stride] = the merged channel columns (out of ivs_interp1d_batch_f64), sym_code [total_queries] =
 * gathered symbol codes (negative = null) or NULL.
 */
int ivs_frame_rows(const int64_t* q_off, int64_t n_series, int64_t total_queries, const int64_t* first_ns,
                   const double* chan, int64_t chan_stride, int32_t n_channels, const int32_t* sym_code,
                   const int32_t* status, const uint8_t* needs, int64_t* date_ns, uint8_t* keep, void* stream);

/*
 * The whole long output frame in ONE pass over its rows (core.py:54-74 for S symbols at once; ABI 3): what the five calls
 * above do together -- ivs_interp1d[_greeks]_batch_f64 on the integer lattice, ivs_ffill_index_batch, ivs_gather_rows_f64 /
 * _i32 and ivs_frame_rows -- without the forward-fill index ever reaching memory: a block owns 1024 consecutive output rows,
 * stages the source rows of its symbols in LDS, a thread walks four consecutive rows (one interval search per thread, not per
 * row and channel) and every column leaves as 16-byte stores.  Same results as the separate calls, bit for bit.
 *
 *   src_pos [total_src], src_off [S+1], q_off [S+1]   as in ivs_ffill_index_batch; src_off is also the CSR of the knots
 *   yk [C][yk_stride], chan_out [C][chan_stride], status [S*C], method          as in ivs_interp1d_batch_f64 (xq = the lattice)
 *   valid [n_valid][valid_stride]                   validity rows (1 = source cell non-null), n_valid <= 16 on the fast path
 *   fsrc [n_f][fsrc_stride] f64 / csrc [n_c][csrc_stride] i32   source columns; f_rows [n_f] / c_rows [n_c] (device) = the
 *                                                   validity row each column forward-fills by; f_out [n_f][f_stride],
 *                                                   c_out [n_c][c_stride] (missing: NaN / -1)
 *   idx_rows [n_idx] (device), idx_out [n_idx][idx_stride]      raw gather index (flat source row or -1) of these validity
 *                                                   rows, for columns the host gathers itself; n_idx may be 0
 *   first_ns [S], needs [S*C], sym_col, date_ns [total_queries], keep [total_queries]   as in ivs_frame_rows; sym_col = the
 *                                                   code column that holds the symbol (its -1 drops the row) or -1;
 *                                                   date_ns == NULL skips both
 *   g_strike / g_rate / g_put, strike_src, rate_src, put_src, ch_*, greeks [5][greeks_stride]   as in
 *                                                   ivs_interp1d_greeks_batch_f64 with validity rows in place of fill_idx
 *                                                   rows; greeks == NULL: no epilogue
 *   workspace   ivs_frame_workspace_bytes(total_src, S, C) bytes
 *
 * Per series: any number of source rows and valid knots gives the same results.  The staged forms of the pass keep knot ranks
 * and counts in 16 bits, so a block that touches a series of more than 65 535 source rows always takes the per-row path on
 * the global arrays (the cost of the separate calls for those blocks); total_src is limited to 2^31 - 1.
 */
typedef struct ivs_frame_args {
    const int64_t* src_pos; const int64_t* src_off; const int64_t* q_off;
    int64_t n_series, total_src, total_queries;
    const double* yk; int64_t yk_stride; int32_t n_channels; int32_t method;
    double* chan_out; int64_t chan_stride; int32_t* status;
    const uint8_t* valid; int64_t valid_stride; int32_t n_valid;
    const double* fsrc; int64_t fsrc_stride; const int32_t* f_rows; int32_t n_f; double* f_out; int64_t f_stride;
    const int32_t* csrc; int64_t csrc_stride; const int32_t* c_rows; int32_t n_c; int32_t* c_out; int64_t c_stride;
    const int32_t* idx_rows; int32_t n_idx; int32_t* idx_out; int64_t idx_stride;
    const int64_t* first_ns; const uint8_t* needs; int32_t sym_col; int64_t* date_ns; uint8_t* keep;
    int32_t g_strike, g_rate, g_put; const double* strike_src; const double* rate_src; const uint8_t* put_src;
    int32_t ch_iv, ch_underlying, ch_ttm; double* greeks; int64_t greeks_stride;
} ivs_frame_args;
size_t ivs_frame_workspace_bytes(int64_t total_src, int64_t n_series, int32_t n_channels);
int ivs_frame_columns_f64(const ivs_frame_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Batch of (strike x maturity) surfaces: strike pass then maturity pass, each pass the
 * 1-D operator above (this repository's documented composition).
 *
 *   K      strikes.  k_off == NULL: surface b at K + b*k_stride (k_stride 0 = one shared grid), nK each.
 *                    k_off != NULL: ragged, surface b has k_off[b+1]-k_off[b] strikes at K + k_off[b];
 *                                   nK is then the maximum count in the batch and k_stride the TOTAL number of strikes
 *                                   K holds (sigma: nT times that): a surface whose span is negative, exceeds nK or
 *                                   leaves [0, k_stride] gets IVS_ST_BAD_SHAPE and is skipped -- no host-side validation
 *                                   of the offsets is needed (0 = total unknown: only the span is checked).
 *   T      maturities of surface b at T + b*t_stride (0 = shared), nT each (nT <= 32)
 *   sigma  surface b at sigma + nT*nK*b (uniform) or sigma + nT*k_off[b] (ragged); [nT][nK_b] row-major
 *   Kq/Tq  query grids of surface b at Kq + b*kq_stride / Tq + b*tq_stride (0 = shared), mK / mT points
 *   out    [B][mT][mK]
 *   status [B] or NULL; IVS_ST_* OR-ed over every 1-D solve of the surface
 *   NaN in sigma = missing quote: the row keeps its own knot set.  64 x 16 batches are probed by the call itself (one row of
 *          64 surfaces spread over the batch): when half of the sampled rows lack a quote -- or at least 5 of them lack about
 *          one quote each: sparse independent gaps, which hit most SURFACES -- every surface goes to the compaction kernel
 *          directly, otherwise the fast kernel tags the few that do and a second pass redoes them -- no flag, same results
 *   flags  0, or IVS_FLAG_FORCE_GENERIC to bypass the dense fast path (testing / A-B timing); bits 8..15 =
 *          IVS_FLAG_MAP_GROUPS(n): tuning override of the surface -> workgroup mapping of the 64x16 kernel (0 = default)
 *   workspace  ivs_surface_workspace_bytes(B, ragged) bytes of device scratch (ragged = k_off != NULL): the
 *          batch-wide maturity tables (read by the kernels through the scalar cache), the work-queue heads and redo
 *          flags of the persistent kernels (zeroed by the call itself, on the caller's stream) and, for ragged batches,
 *          the per-size-class work lists.  Contents are undefined after the call; calls that may overlap in time (other
 *          streams, other threads) need distinct workspaces, calls on one stream may share one.
 */
enum { IVS_FLAG_FORCE_GENERIC = 1, IVS_FLAG_ONE_PASS = 2 /* testing / A-B timing: skip the row-pass kernels (one-pass dense kernels instead) */ };
#define IVS_FLAG_MAP_GROUPS(n) (((n) & 0xff) << 8)
size_t ivs_surface_workspace_bytes(int64_t B, int32_t ragged);
int ivs_surface_batch_f64(const double* K, const int64_t* k_off, int64_t k_stride, int32_t nK,
                          const double* T, int64_t t_stride, int32_t nT,
                          const double* sigma, int64_t B,
                          const double* Kq, int64_t kq_stride, int32_t mK,
                          const double* Tq, int64_t tq_stride, int32_t mT,
                          double* out, int32_t* status, int32_t method, int32_t flags,
                          void* workspace, size_t workspace_bytes, void* stream);

/*
 * Per-minute surface snapshots of ONE underlying from its interpolated option chain (ABI 4; DESIGN.md section 8, rules
 * S1-S8): the input of ivs_surface_batch_f64 -- sigma, T and the strike query grid of every minute -- assembled on the device
 * from the rows of `interpolated_trading_tickers`.  The host does the per-contract bookkeeping (symbol parsing, expiry
 * instants, the strike axis, the cell table); the kernel reads every row once and writes every cell once:
 *
 *   date_ns, iv, underlying [n_rows]   the rows of the underlying's C contracts, contract after contract (CSR row_off [C+1]),
 *                                      sorted by date inside a contract (ties in input order)
 *   cells [nT*nK][2] (int32)           contract of cell e*nK + k: [0] the call, [1] the put, -1 = none
 *   strike [nK]                        the strike axis (ascending); expiry_ns [nT] = E_e, ascending
 *   t0_ns, n_snapshots                 snapshot b is the minute [t0 + b*60 s, t0 + (b+1)*60 s)
 *   sigma [B][nT][nK]                  S5/S6: the last row of the minute per contract (NaN iv = absent); both sides -> the put
 *                                      iff strike < the put row's underlying price, else the call; NaN where no side is
 *                                      present or the expiry has passed (T <= 0)
 *   T [B][nT]                          (E_e - t_b) / (365 days), also for passed expiries
 *   spot [B], quotes [B] (int32)       S7: the underlying price of the row behind the first quoted cell in (expiry, strike)
 *                                      order (NaN if none), the number of quoted cells
 *   moneyness [mK], kq_empty, Kq [B][mK]   optional (Kq == NULL skips): Kq[b] = spot[b] * moneyness, or kq_empty *
 *                                      moneyness where spot[b] is NaN
 * Every output element is written, bitwise deterministically (plain stores, no atomics).  nT <= 32 (the surface engine's
 * limit) and int32 tables (C, nT*nK, B / minute tile) are checked: IVS_ERANGE.  No workspace.
 */
typedef struct ivs_snapshot_args {
    const int64_t* date_ns; const double* iv; const double* underlying; int64_t n_rows;
    const int64_t* row_off; int64_t n_contracts;
    const int32_t* cells; const double* strike; const int64_t* expiry_ns; int32_t nT, nK;
    int64_t t0_ns, n_snapshots;
    const double* moneyness; int32_t mK; double kq_empty;
    double* sigma; double* T; double* spot; int32_t* quotes; double* Kq;
} ivs_snapshot_args;
int ivs_snapshot_assemble_f64(const ivs_snapshot_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Delta-quoted smile points off snapshot surfaces (ABI 5; DESIGN.md section 9, rules D1-D7): the at-the-money and the
 * 25- / 10-delta call and put vols a desk quotes, read off the `out` of ivs_surface_batch_f64 on the device.  For every
 * row (b, j) and every target the kernel inverts Black-Scholes call delta -> (strike, vol) on the chord between the first
 * pair of neighbouring valid nodes that brackets the target:
 *
 *   vol [B][mT][mK]                    the surfaces (out of ivs_surface_batch_f64); a node with a non-finite or <= 0 vol or
 *                                      strike is skipped (its neighbours pair up across it)
 *   Kq, kq_stride / Tq, tq_stride      strike and tenor grids of snapshot b at Kq + b*kq_stride / Tq + b*tq_stride
 *                                      (0 = one shared grid), mK / mT points, strikes ascending
 *   spot [B], rate                     S of snapshot b and the scalar interest rate of d1 (0.0 = the schema default);
 *                                      d1 is ivs_bs_greeks_f64's: (log(S/K) + (r + sigma^2/2) T) / (sigma sqrt(T))
 *   z [nD] (HOST)                      targets as z = inv_cdf(call delta) (a put delta d means the call delta 1 + d; ATM
 *                                      = 0.5 -> z = 0); 1 <= nD <= 16; copied into the kernel arguments by the call
 *   q_vol, q_strike [B][mT][nD]        vol and strike where d1 - z changes sign, by 52 bisection steps on the chord
 *   q_flags [B][mT][nD] (int32)        IVS_SM_*: NO_CROSSING and DEAD leave NaN in q_vol / q_strike; AMBIGUOUS = more than
 *                                      one bracket, the lowest-strike one was used; DEAD = spot[b] or the tenor is not a
 *                                      finite positive number or the row has fewer than 2 valid nodes
 * Every output element is written, bitwise deterministically (plain stores, no atomics), in ONE launch.  mK >= 2 and
 * B*mT < 2^31 are checked (IVS_ERANGE); B == 0 or mT == 0 is a no-op.  No workspace.
 * rows_per_wave: how many consecutive rows one wavefront takes (their rows x nD inversions share its 64 lanes); 0 lets the
 * call choose by batch size, 1..64/nD forces it (IVS_ERANGE outside).  The results do not depend on it, bit for bit.
 */
enum {
    IVS_SM_OK          = 0,
    IVS_SM_NO_CROSSING = 1,
    IVS_SM_AMBIGUOUS   = 2,
    IVS_SM_DEAD        = 4
};
typedef struct ivs_smile_args {
    const double* vol;
    const double* Kq; int64_t kq_stride;
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* z; /* host */
    int32_t mK, mT, nD; int64_t B;
    double* q_vol; double* q_strike; int32_t* q_flags;
    int32_t rows_per_wave; /* 0 = chosen by the call; 1..64/nD = tuning / testing override, same results */
} ivs_smile_args;
int ivs_smile_delta_points_f64(const ivs_smile_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Static-arbitrage report, risk-neutral density and Dupire local volatility off snapshot surfaces (DESIGN.md section 10,
 * rules A1-A8; additive to ABI 5).  A 5-point stencil in (ln k, tau) over the total variance w = vol^2 tau of every node
 * of `vol` (the `out` of ivs_surface_batch_f64), with the inputs of ivs_smile_delta_points_f64:
 *
 *   vol [B][mT][mK], Kq / kq_stride, Tq / tq_stride, spot [B], rate      as for the smile points; a stride is 0 (one
 *                                      shared grid) or mK / mT (one grid per snapshot)
 *   flags [B][mT][mK] (int32)          IVS_AR_*: DEAD = the node's vol or strike, the snapshot's spot or the row's tenor is
 *                                      not a finite positive number; NO_STENCIL = a strike neighbour is missing or
 *                                      invalid, a strike spacing is not > 0, or no tenor neighbour counts; otherwise
 *                                      CALENDAR (Dupire numerator N < 0) | BUTTERFLY (density factor g < 0), 0 = clean
 *   counts [B][4] (int32)              nodes evaluated (neither DEAD nor NO_STENCIL), CALENDAR nodes, BUTTERFLY nodes,
 *                                      nodes with a finite local vol
 *   worst [B][2]                       min N and min g over the evaluated nodes, NaN if there are none
 *   local_vol, density [B][mT][mK]     optional (NULL = not written): sqrt(N / g) where N >= 0 and g > 0, and the
 *                                      undiscounted d2C/dK2 (negative where g is); NaN at DEAD / NO_STENCIL nodes
 * Every element of every requested output is written, bitwise deterministically (plain stores, no atomics), in ONE
 * launch.  mK >= 3, mT >= 2 and B*mT < 2^31 are checked (IVS_ERANGE); B == 0 is a no-op.  No workspace.
 */
enum {
    IVS_AR_CALENDAR   = 1,
    IVS_AR_BUTTERFLY  = 2,
    IVS_AR_NO_STENCIL = 4,
    IVS_AR_DEAD       = 8
};
typedef struct ivs_arbitrage_args {
    const double* vol;
    const double* Kq; int64_t kq_stride;
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    int32_t mK, mT; int64_t B;
    int32_t* flags; int32_t* counts; double* worst;
    double* local_vol; double* density; /* either may be NULL */
} ivs_arbitrage_args;
int ivs_surface_arbitrage_f64(const ivs_arbitrage_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Model-free variance, skew, kurtosis and a constant-maturity volatility index off snapshot surfaces (DESIGN.md section
 * 11, rules M1-M8; additive to ABI 5).  Per row (b, j) of `vol` the trapezoid over its valid strikes of g(x) Q / k^2, with
 * Q the undiscounted out-of-the-money Black price at the node's vol and x = ln(k / F), F = spot exp(rate tau), and with
 * the inputs of ivs_surface_arbitrage_f64:
 *
 *   vol [B][mT][mK], Kq / kq_stride, Tq / tq_stride, spot [B], rate      as for the arbitrage report; a stride is 0 (one
 *                                      shared grid) or mK / mT (one grid per snapshot)
 *   min_mass                           in [0, 1]: a row whose strikes cover less lognormal probability gets TRUNCATED
 *                                      (0 = never)
 *   horizons [nH] (HOST)               index horizons in years, finite and > 0; 0 <= nH <= 8; copied into the kernel
 *                                      arguments by the call
 *   raw [B][mT][4]                     the contracts L (log contract = index^2 tau), V, W, X (g = 2, 2(1 - x), 6x - 3x^2,
 *                                      12x^2 - 4x^3)
 *   stats [B][mT][4]                   mf_vol = sqrt(L / tau), bkm_vol = sqrt(var / tau), skew, kurt, with
 *                                      mu = -V/2 - W/6 - X/24 and var = V - mu^2
 *   mass [B][mT]                       the lognormal probability between the first and the last valid strike
 *   flags [B][mT] (int32)              IVS_MM_*: DEAD = spot[b] or the tenor is not a finite positive number, fewer than 2
 *                                      valid nodes, valid strikes not strictly ascending, or L <= 0 or var <= 0 (NaN in
 *                                      every value of the row); ONE_SIDED = F outside the valid strikes; TRUNCATED = mass <
 *                                      min_mass; HOLES = an invalid node between two valid ones was skipped
 *   index [B][nH], index_flags [B][nH] (int32)    100 sqrt(L_h / h), L_h linear in tau between the first pair of consecutive
 *                                      rows that are not DEAD and bracket h; the OR of the two rows' flags, or NaN and
 *                                      NO_BRACKET; both NULL with nH == 0 (neither is touched then)
 * Every element of every output is written, bitwise deterministically (plain stores, no atomics), in ONE launch.  mK >= 2,
 * mT <= 512, nH <= 8 and B*mT < 2^31 are checked (IVS_ERANGE); B == 0 or mT == 0 is a no-op.  No workspace.
 * snapshots_per_wg: how many consecutive snapshots one workgroup takes; 0 lets the call choose, 1..4 forces it
 * (IVS_ERANGE outside).  The results do not depend on it, bit for bit.
 */
enum {
    IVS_MM_ONE_SIDED  = 1,
    IVS_MM_TRUNCATED  = 2,
    IVS_MM_HOLES      = 4,
    IVS_MM_DEAD       = 8,
    IVS_MM_NO_BRACKET = 16
};
typedef struct ivs_moments_args {
    const double* vol;
    const double* Kq; int64_t kq_stride;
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate; double min_mass;
    const double* horizons; /* host */ int32_t nH;
    int32_t mK, mT; int64_t B;
    double* raw;     /* [B][mT][4]  L, V, W, X */
    double* stats;   /* [B][mT][4]  mf_vol, bkm_vol, skew, kurt */
    double* mass;    /* [B][mT] */
    int32_t* flags;  /* [B][mT] */
    double* index; int32_t* index_flags; /* [B][nH]; both NULL with nH == 0: no M7 */
    int32_t snapshots_per_wg; /* 0 = chosen by the call; 1..4 tuning / testing override, same bits */
} ivs_moments_args;
int ivs_surface_moments_f64(const ivs_moments_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Raw SVI slices off snapshot surfaces, with a butterfly check (rules V1-V9; additive to ABI 5).  Per
 * row (b, j) of `vol` the least-squares fit of w(x) = a + b (rho (x - m) + sqrt((x - m)^2 + sigma^2)) to the total variances
 * w = vol^2 tau at x = ln(k / spot) - rate tau of the row's valid nodes: a fixed number of rounds of an 8 x 8 grid search over
 * (m, ln sigma), each candidate's (a, b, rho) from the exactly solved constrained linear problem (0 <= a <= max w,
 * |rho| <= 1, b (1 + |rho|) <= 2).  Deterministic, no data-dependent loop counts.  With the inputs of
 * ivs_surface_moments_f64:
 *
 *   vol [B][mT][mK], Kq / kq_stride, Tq / tq_stride, spot [B], rate      as for the moments; a stride is 0 (one shared grid)
 *                                      or mK / mT (one grid per snapshot)
 *   rounds                             rounds of the grid search; 0 = the default 16, 1..24 otherwise.  A round shrinks the
 *                                      box to 2/7 of its width
 *   params [B][mT][5]                  a, b, rho, m, sigma
 *   fit [B][mT][4]                     rmse_w = sqrt(SSE / n) in total variance; rmse_vol and max_vol_err of the fitted vol
 *                                      sqrt(w_fit / tau) against vol over the valid nodes; g_min = the minimum over the valid
 *                                      nodes of Durrleman's g(x) = (1 - x w'/(2w))^2 - (w'^2/4)(1/w + 1/4) + w''/2 on the
 *                                      fitted curve
 *   flags [B][mT] (int32)              IVS_SV_*: DEAD (alone, NaN in every value of the row and in its `fitted` row) = spot[b]
 *                                      or the tenor is not a finite positive number, fewer than 5 valid nodes, or valid
 *                                      strikes not strictly ascending; HOLES = an invalid node between two valid ones was
 *                                      skipped; BOUND = a constraint of the linear problem is active; EDGE = m or ln sigma
 *                                      ended on a border of its domain ([first x, last x], [ln(X/256), ln(4X)], X = last x
 *                                      - first x) or within 2^-20 of the domain's width of it; BUTTERFLY = g_min < 0; DEGENERATE = the fitted w is <= 0 at a valid node
 *                                      (fitted vol 0 there, g_min NaN)
 *   fitted [B][mT][mK] or NULL         the fitted vol at every node whose strike is a finite positive number, valid vol or
 *                                      not (holes are filled); NaN elsewhere.  NULL: not computed, nothing is touched
 * Every element of every requested output is written, bitwise deterministically (plain stores, no atomics), in ONE launch.
 * 5 <= mK <= 1024, rounds, rows_per_wg and B*mT < 2^31 are checked (IVS_ERANGE); B == 0 or mT == 0 is a no-op.  No workspace.
 * rows_per_wg: how many rows one workgroup takes, one per wavefront; 0 lets the call choose, 1..4 forces it.  The results
 * do not depend on it, bit for bit.
 */
enum {
    IVS_SV_BOUND      = 1,
    IVS_SV_EDGE       = 2,
    IVS_SV_HOLES      = 4,
    IVS_SV_DEAD       = 8,
    IVS_SV_BUTTERFLY  = 16,
    IVS_SV_DEGENERATE = 32
};
typedef struct ivs_svi_args {
    const double* vol;
    const double* Kq; int64_t kq_stride;
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    int32_t mK, mT; int64_t B;
    int32_t rounds;  /* 0 = 16 */
    double* params;  /* [B][mT][5]  a, b, rho, m, sigma */
    double* fit;     /* [B][mT][4]  rmse_w, rmse_vol, max_vol_err, g_min */
    int32_t* flags;  /* [B][mT] */
    double* fitted;  /* [B][mT][mK], may be NULL */
    int32_t rows_per_wg; /* 0 = chosen by the call; 1..4 tuning / testing override, same bits */
} ivs_svi_args;
int ivs_svi_slices_f64(const ivs_svi_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Risk-neutral distribution off the raw SVI slices: quantiles and probabilities (rules P1-P9; additive
 * to ABI 5).  Per row (b, j) of `params` (the `params` of ivs_svi_slices_f64) the closed-form risk-neutral CDF of the slice
 * w(x) = a + b (rho (x - m) + sqrt((x - m)^2 + sigma^2)), x = ln(K / F), F = spot exp(rate tau):
 * L(x) = P(S_tau <= F e^x) = Phi(-d2) + phi(d2) theta'(x) and U = 1 - L = Phi(d2) - phi(d2) theta'(x), theta = sqrt(w),
 * d2 = -x / theta - theta / 2.  A 64-point scan grid x_i = s0 y_i (s0 = theta(0), y_i = j (1 + j^2/64) / 8, j = i - 31.5,
 * span +- 64.98 s0) brackets every target; 52 bisection steps invert it.  Deterministic, no data-dependent loop counts.
 *
 *   params [B][mT][5]                  a, b, rho, m, sigma.  A row is DEAD unless spot[b] and the tenor are finite and > 0, the
 *                                      five parameters are finite, b >= 0, |rho| <= 1, sigma > 0 and a + b sigma sqrt(1 - rho^2)
 *                                      > 0 (the DEAD rows of ivs_svi_slices_f64 carry NaN and so are DEAD here)
 *   Tq, tq_stride / spot [B], rate     tenor grid of snapshot b at Tq + b*tq_stride (0 = one shared grid, else mT), S of
 *                                      snapshot b, the scalar interest rate of the forward
 *   probs [nP] (HOST)                  target probabilities, each strictly inside (0, 1); 1 <= nP <= 16; copied into the
 *                                      kernel arguments by the call.  p <= 0.5 solves L(x) = p, p > 0.5 solves U(x) = 1 - p
 *   levels [nL] (HOST)                 moneyness levels u (K = spot u), finite and > 0; 0 <= nL <= 16; copied likewise
 *   max_tail                           in [0, 1]: the row gets TAILS when a tail of the scan grid exceeds it in magnitude
 *   q_x, q_strike [B][mT][nP]          the quantile as x* = ln(K / F) and as the strike F exp(x*)
 *   q_flags [B][mT][nP] (int32)        0, or IVS_DS_NO_BRACKET (no grid interval with h < 0 then h >= 0: NaN outputs),
 *                                      IVS_DS_AMBIGUOUS (more than one: the first was used; the CDF is not monotone, a
 *                                      butterfly arbitrage of the fit), IVS_DS_DEAD (the row is: NaN outputs)
 *   p_below, p_above [B][mT][nL]       L and U at x = log(u) - rate tau; both NULL with nL == 0 (neither is touched then)
 *   tails [B][mT][2]                   L(x_0) and U(x_63): the probability the scan grid leaves out on either side
 *   flags [B][mT] (int32)              0, IVS_DS_TAILS (|L(x_0)| or |U(x_63)| > max_tail) or IVS_DS_DEAD (alone; NaN in every
 *                                      value of the row)
 * Every element of every output is written, bitwise deterministically (plain stores, no atomics), in ONE launch.  nP, nL,
 * rows_per_wave and B*mT < 2^31 are checked (IVS_ERANGE); a probability outside (0, 1), a level that is not finite and > 0, a
 * max_tail outside [0, 1] or a stride that is neither 0 nor mT is IVS_EINVAL; B == 0 or mT == 0 is a no-op.  No workspace, no
 * allocation, no synchronisation (capturable).
 * rows_per_wave: how many consecutive rows one wavefront takes (their rows x nP inversions share its 64 lanes); 0 lets the
 * call choose by batch size, 1..64/nP forces it (IVS_ERANGE outside).  The results do not depend on it, bit for bit.
 */
enum {
    IVS_DS_NO_BRACKET = 1,
    IVS_DS_AMBIGUOUS  = 2,
    IVS_DS_TAILS      = 4,
    IVS_DS_DEAD       = 8
};
typedef struct ivs_distribution_args {
    const double* params; /* [B][mT][5]  a, b, rho, m, sigma */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate; double max_tail;
    const double* probs; /* host */ int32_t nP;
    const double* levels; /* host */ int32_t nL;
    int32_t mT; int64_t B;
    double* q_x; double* q_strike; int32_t* q_flags; /* [B][mT][nP] */
    double* p_below; double* p_above;                /* [B][mT][nL]; both NULL with nL == 0 */
    double* tails;   /* [B][mT][2]  L(x_0), U(x_63) */
    int32_t* flags;  /* [B][mT] */
    int32_t rows_per_wave; /* 0 = chosen by the call; 1..64/nP = tuning / testing override, same bits */
} ivs_distribution_args;
int ivs_svi_distribution_f64(const ivs_distribution_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * SVI term structure: a calendar check between the slices of a snapshot and the surface at any (strike, expiry) (DESIGN.md
 * section 14, rules T1-T4, C1-C6, E1-E6; additive to ABI 5).  Both read `params` [B][mT][5] (the `params` of
 * ivs_svi_slices_f64), Tq / tq_stride (0 = one shared grid, else mT) and spot [B]; mT <= 64.  A row is live by the rule of
 * ivs_svi_distribution_f64.  The live rows of a snapshot must have strictly ascending tenors; otherwise the snapshot is
 * UNORDERED: every value of it is NaN and every flag of it is that flag alone.  w, w', w'' are those of the slice
 * w(x) = a + b (rho (x - m) + sqrt((x - m)^2 + sigma^2)), x = ln(K / F).  Deterministic, no data-dependent loop counts.
 *
 * ivs_svi_calendar_f64: entry j of every output describes the pair (j, j'), j' the lowest live row above j.  A dead row gets
 * IVS_SC_DEAD, the last live row IVS_SC_LAST, both NaN values and n_cross = 0.  d(x) = w_j'(x) - w_j(x) on the grid
 * x_i = s0 y_i, s0 = sqrt(max(w_j(0), w_j'(0))), y_i = t (1 + t^2/1024) / 8, t = i - 31.5, i = 0..63 (span +- 7.75 s0), and
 * at m_j and m_j' (points 64, 65):
 *   d_min, x_min [B][mT]               the minimum of d over the 66 points (ties to the lowest index; a NaN compares as +inf)
 *                                      and its x
 *   d_atm [B][mT]                      d(0)
 *   n_cross [B][mT] (int32)            grid cells i < 63 with (d(x_i) < 0) != (d(x_i+1) < 0)
 *   x_cross [B][mT][2]                 the first and the last of those crossings, each by 52 bisection steps from its cell;
 *                                      NaN without a crossing, twice the same with exactly one
 *   flags [B][mT] (int32)              IVS_SC_CALENDAR = d_min < 0; IVS_SC_WING_LEFT = b'(1 - rho') < b(1 - rho) and
 *                                      IVS_SC_WING_RIGHT = b'(1 + rho') < b(1 + rho): the later slice ends below the
 *                                      earlier one beyond any grid; DEAD, LAST, UNORDERED alone
 * rows_per_wave: how many consecutive rows one wavefront takes; 0 lets the call choose, 1..32 forces it (IVS_ERANGE
 * outside).  The results do not depend on it, bit for bit.
 *
 * ivs_svi_eval_f64: Q queries (u, tau) per snapshot at u + b*q_stride, tau + b*q_stride (q_stride 0 = one shared list, else
 * Q).  K = spot u (strike_mode 0) or K = u (strike_mode 1); F = spot exp(rate tau), x = log(K / spot) - rate tau,
 * D = exp(-rate tau).  A query is IVS_SE_DEAD (NaN) unless u, tau and spot are finite and > 0 and the snapshot has a live row.
 * lo = the last live row with tenor <= tau, hi = the first with tenor > tau; total variance, w' and w'' linear in the tenor
 * between the two at fixed x; before the first live row that row scaled by tau / tenor (IVS_SE_SHORT), without a row above
 * the last one likewise (IVS_SE_LONG).
 *   w, vol [B][Q]                      W and sqrt(W / tau)
 *   call, put [B][Q]                   D (F Phi(d1) - K Phi(d2)) and D (K Phi(-d2) - F Phi(-d1)), d1 = -x/theta + theta/2,
 *                                      d2 = d1 - theta, theta = sqrt(W)
 *   fwd_var [B][Q]                     V = (w_hi - w_lo) / (tenor_hi - tenor_lo) at fixed x; w / tenor under SHORT / LONG
 *   g [B][Q]                           (1 - x W'/(2W))^2 - (W'^2/4)(1/W + 1/4) + W''/2
 *   local_vol [B][Q]                   sqrt(V / g); NaN with IVS_SE_NEG_FWD (V < 0) or IVS_SE_NEG_G (g <= 0)
 *   flags [B][Q] (int32)               IVS_SE_*; required.  Each of the seven value outputs may be NULL: it is then neither
 *                                      computed nor written
 * Every element of every requested output is written, bitwise deterministically (plain stores, no atomics), in ONE launch.
 * IVS_EINVAL: null args or a null required pointer, a negative size, a stride that is neither 0 nor the full size, a
 * strike_mode that is not 0 or 1; IVS_ERANGE: mT > 64, rows_per_wave outside 0..32, B*mT or B*Q >= 2^31; B == 0, mT == 0 or
 * Q == 0 is a no-op.  No workspace, no allocation, no synchronisation (capturable).
 */
enum {
    IVS_SC_CALENDAR   = 1,
    IVS_SC_WING_LEFT  = 2,
    IVS_SC_WING_RIGHT = 4,
    IVS_SC_DEAD       = 8,
    IVS_SC_LAST       = 16,
    IVS_SC_UNORDERED  = 32
};
enum {
    IVS_SE_SHORT      = 1,
    IVS_SE_LONG       = 2,
    IVS_SE_NEG_FWD    = 4,
    IVS_SE_DEAD       = 8,
    IVS_SE_NEG_G      = 16,
    IVS_SE_UNORDERED  = 32
};
typedef struct ivs_calendar_args {
    const double* params; /* [B][mT][5]  a, b, rho, m, sigma */
    const double* Tq; int64_t tq_stride;
    const double* spot;
    int32_t mT; int64_t B;
    double* d_min; double* x_min; double* d_atm; /* [B][mT] */
    double* x_cross;  /* [B][mT][2] */
    int32_t* n_cross; int32_t* flags; /* [B][mT] */
    int32_t rows_per_wave; /* 0 = chosen by the call; 1..32 = tuning / testing override, same bits */
} ivs_calendar_args;
int ivs_svi_calendar_f64(const ivs_calendar_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

typedef struct ivs_eval_args {
    const double* params; /* [B][mT][5]  a, b, rho, m, sigma */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* u; const double* tau; int64_t q_stride; /* [Q] (stride 0) or [B][Q] (stride Q) */
    int32_t strike_mode; /* 0: K = spot u; 1: K = u */
    int32_t mT; int64_t Q; int64_t B;
    double* w; double* vol; double* call; double* put; double* fwd_var; double* g; double* local_vol; /* [B][Q], each may be NULL */
    int32_t* flags;   /* [B][Q] */
} ivs_eval_args;
int ivs_svi_eval_f64(const ivs_eval_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Arbitrage-free SSVI surface per snapshot, fitted jointly across tenors (rules J1-J8; additive to ABI
 * 5).  One (rho, eta, gamma) per snapshot and one ATM total variance theta_j per tenor:
 * w_j(x) = theta_j / 2 (1 + rho phi_j x + sqrt((phi_j x + rho)^2 + 1 - rho^2)), phi_j = eta theta_j^-gamma, fitted to the total
 * variances w = vol^2 tau at x = ln(k / spot) - rate tau of every valid node of every live row, in least squares of
 * (w_fit - w) / theta_j.  theta_j is the running maximum of theta0 in tenor order (no calendar arbitrage), gamma stays in [0, 1]
 * and eta = exp(s) eta_max with s <= 0, eta_max the largest eta with theta phi (1 + |rho|) <= 4 and theta phi^2 (1 + |rho|) <= 4 on
 * every slice (no butterfly arbitrage).  A fixed number of rounds of a 6 x 6 x 6 grid search over rho in [-1 + 2^-10, 1 - 2^-10],
 * gamma in [0, 1], s in [ln 2^-10, 0]; deterministic, no data-dependent loop counts.  With the inputs of ivs_svi_slices_f64:
 *
 *   vol [B][mT][mK], Kq / kq_stride, Tq / tq_stride, spot [B], rate      as there; the valid strikes need not ascend
 *   raw [B][mT][5] or theta0 [B][mT]   where theta0 comes from, exactly one non-NULL: theta0 itself, or raw SVI slices (the
 *                                      `params` of ivs_svi_slices_f64), theta0 = w_j(0) of a slice that is live by the rule of
 *                                      ivs_svi_distribution_f64, NaN otherwise
 *   rounds                             rounds of the grid search; 0 = the default 20, 1..32 otherwise.  A round shrinks the
 *                                      box to 2/5 of its width
 *   surface [B][4]                     rho, eta, gamma, rmse = sqrt(SSE / n) of the relative residuals
 *   theta [B][mT]                      theta_j
 *   params [B][mT][5]                  the slice in raw SVI form: a = theta (1 - rho^2) / 2, b = theta phi / 2, rho,
 *                                      m = -rho / phi, sigma = sqrt(1 - rho^2) / phi
 *   fit [B][mT][3]                     rmse_vol and max_vol_err of the fitted vol sqrt(w_fit / tau) against vol over the row's
 *                                      valid nodes, g_min = the minimum there of Durrleman's g on the raw form; NaN for a live
 *                                      row without a valid node
 *   flags [B][mT] (int32)              IVS_SS_*: DEAD (alone, NaN in every value of the row) = spot[b], the tenor or theta0 is
 *                                      not a finite positive number, or the snapshot is SURF_DEAD or UNORDERED; HOLES = an
 *                                      invalid node between two valid ones; RAISED = theta_j > theta0_j; BUTTERFLY = g_min < 0
 *                                      (a guard against rounding, not a regular outcome)
 *   sflags [B] (int32)                 IVS_SF_*: SURF_DEAD = no live row or fewer than 5 valid nodes on the live rows;
 *                                      UNORDERED = the live tenors do not ascend strictly (both: NaN in every value of the
 *                                      snapshot); EDGE_RHO, EDGE_GAMMA, EDGE_ETA_LOW = the final point lies on that border or
 *                                      within 2^-20 of the domain's width of it; AT_BOUND = s within that band of 0: eta sits
 *                                      on the butterfly bound
 *   fitted [B][mT][mK] or NULL         the fitted vol at every node whose strike is a finite positive number; NaN elsewhere.
 *                                      NULL: not computed, nothing is touched
 * Every element of every requested output is written, bitwise deterministically (plain stores, no atomics), in ONE launch of
 * one workgroup per snapshot.  IVS_EINVAL: null args or a null required pointer, both or neither of raw / theta0, a negative
 * size, a stride that is neither 0 nor the full size; IVS_ERANGE: mT > 64, mK < 1, mT*mK > 3072 (the valid nodes of a snapshot
 * live in LDS), rounds outside 0..32, B*mT*mK >= 2^31; B == 0 or mT == 0 is a no-op.  No workspace, no allocation, no
 * synchronisation (capturable).
 */
enum {
    IVS_SS_RAISED     = 1,
    IVS_SS_HOLES      = 4,
    IVS_SS_DEAD       = 8,
    IVS_SS_BUTTERFLY  = 16
};
enum {
    IVS_SF_EDGE_RHO     = 1,
    IVS_SF_EDGE_GAMMA   = 2,
    IVS_SF_EDGE_ETA_LOW = 4,
    IVS_SF_SURF_DEAD    = 8,
    IVS_SF_AT_BOUND     = 16,
    IVS_SF_UNORDERED    = 32
};
typedef struct ivs_ssvi_args {
    const double* vol;
    const double* Kq; int64_t kq_stride;
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* raw;    /* [B][mT][5] or NULL */
    const double* theta0; /* [B][mT] or NULL */
    int32_t mK, mT; int64_t B;
    int32_t rounds;   /* 0 = 20 */
    double* surface;  /* [B][4]  rho, eta, gamma, rmse */
    double* theta;    /* [B][mT] */
    double* params;   /* [B][mT][5]  a, b, rho, m, sigma */
    double* fit;      /* [B][mT][3]  rmse_vol, max_vol_err, g_min */
    int32_t* flags;   /* [B][mT] */
    int32_t* sflags;  /* [B] */
    double* fitted;   /* [B][mT][mK], may be NULL */
} ivs_ssvi_args;
int ivs_ssvi_surface_f64(const ivs_ssvi_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Book risk off the raw SVI slices: smile-aware Greeks per option, net Greeks and a scenario P&L grid per snapshot (DESIGN.md
 * section 17, rules G0-G6, B1-B5; additive to ABI 5).  Both calls read params / Tq / tq_stride / spot / rate / u / tau /
 * q_stride / strike_mode exactly as ivs_svi_eval_f64 does and place an option on the surface by its rules: K, x, D, W, W', W'',
 * V and the flags IVS_SE_SHORT, LONG, DEAD, UNORDERED.  is_put [Q] (uint8, 1 = put, one list for all snapshots) or NULL = all
 * calls.  With theta = sqrt(W), theta' = W'/(2 theta), theta'' = W''/(2 theta) - W'^2/(4 theta^3), d1 = -x/theta + theta/2,
 * d2 = d1 - theta, d1x = -1/theta + (x/theta^2 + 1/2) theta', d2x = d1x - theta', S = spot:
 *
 * ivs_svi_greeks_f64, each value [B][Q] and each may be NULL (then neither computed nor written):
 *   price                              call S Phi(d1) - K D Phi(d2), put K D Phi(-d2) - S Phi(-d1)
 *   delta_ss, gamma_ss                 sticky strike: Phi(d1) (put: -Phi(-d1)) and phi(d1) / (S theta)
 *   delta_sm, gamma_sm                 sticky moneyness (the curve in x is fixed): delta_ss - phi(d1) theta' and
 *                                      phi(d1) (-d2x - d1 d1x theta' + theta'' - theta') / S
 *   vega                               S phi(d1) sqrt(tau), per unit of vol for a parallel shift
 *   theta                              per year, -d price / d tau at fixed K and S: -S [+-rate (K D / S) Phi(+-d2) +
 *                                      phi(d1) (V - rate W') / (2 theta)], + for a call, - for a put
 *   flags [B][Q] (int32)               IVS_SE_SHORT, LONG, NEG_FWD (V < 0; theta is still the formula's value), DEAD,
 *                                      UNORDERED; required.  A dead option has NaN values.
 *
 * ivs_svi_book_f64: besides qty [Q] (one list for all snapshots; an option whose quantity is not finite is dead too), nA spot
 * shocks a and nV vol shocks v (host arrays).  Cell (i, k): S' = S (1 + a_i), x' = log(K / S') - rate tau, vol
 * sqrt(W(x) / tau) + v_k (sticky strike) or sqrt(W(x') / tau) + v_k (sticky moneyness, the option's bracket and weight
 * unchanged), theta' = vol sqrt(tau), the price formula above at (S', x', theta').  The base price P of the P&L is that of the
 * cell with both shocks zero.
 *   net [B][8]                         sum over the live options of qty x (price, delta_ss, delta_sm, gamma_ss, gamma_sm,
 *                                      vega, theta) and, in slot 7, of |qty| x price
 *   n_dead [B] (int32)                 the dead options; they contribute nothing
 *   pnl_ss, pnl_sm [B][nA][nV]         sum of qty (P' - P) over the live options; either may be NULL.  Exactly +0.0 where
 *                                      a_i == 0 and v_k == 0
 *   cell_flags [B][nA][nV] (int32)     IVS_SB_NEG_VOL_SS / _SM: a live option has a shocked vol <= 0 in the cell under that
 *                                      dynamic; the cell's value is then NaN.  Required.  The bit of a dynamic whose pnl output is
 *                                      NULL is not formed (it is skipped with that dynamic's arithmetic) and stays 0.
 * An UNORDERED snapshot or one without a live slice has NaN in every net and pnl entry, n_dead = Q and cell flags 0.
 * Every sum is formed without atomics in an order that depends on Q alone (an xor butterfly over the 64 lanes of a wavefront,
 * four wavefronts as (s0 + s1) + (s2 + s3), passes of 256 options in turn): the bits do not depend on B, on cells_per_wg or on
 * the run.  cells_per_wg: how many cells one workgroup takes; 0 lets the call choose, 1..256 forces it.
 *
 * IVS_EINVAL: null args or a null required pointer, a negative size, a stride that is neither 0 nor the full size, a
 * strike_mode that is not 0 or 1; IVS_ERANGE: mT > 64, nA or nV > 64, nA nV > 1024, cells_per_wg outside 0..256, a spot shock
 * that is not finite or <= -1, a vol shock that is not finite, B*mT, B*Q or B*nA*nV >= 2^31.  B == 0, mT == 0 or Q == 0 is a
 * no-op for both (nothing is written: the caller defines what an empty book is worth; engine.svi_book fills zeros); the
 * limits above and the shocks are checked before that, so a zero-size call with a bad shock is refused all the same.  With
 * nA nV == 0 net and n_dead are still written.  A refused call
 * launches nothing.  No workspace, no allocation, no synchronisation (capturable); ONE launch each.
 */
enum {
    IVS_SB_NEG_VOL_SS = 1,
    IVS_SB_NEG_VOL_SM = 2
};
typedef struct ivs_greeks_args {
    const double* params; /* [B][mT][5]  a, b, rho, m, sigma */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* u; const double* tau; int64_t q_stride; /* [Q] (stride 0) or [B][Q] (stride Q) */
    const uint8_t* is_put; /* [Q] or NULL */
    int32_t strike_mode; /* 0: K = spot u; 1: K = u */
    int32_t mT; int64_t Q; int64_t B;
    double* price; double* delta_ss; double* delta_sm; double* gamma_ss; double* gamma_sm; double* vega; double* theta; /* [B][Q], each may be NULL */
    int32_t* flags;   /* [B][Q] */
} ivs_greeks_args;
int ivs_svi_greeks_f64(const ivs_greeks_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

typedef struct ivs_book_args {
    const double* params; /* [B][mT][5] */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* u; const double* tau; int64_t q_stride;
    const uint8_t* is_put; /* [Q] or NULL */
    const double* qty;     /* [Q] */
    int32_t strike_mode;
    int32_t mT; int64_t Q; int64_t B;
    const double* spot_shocks; /* host */ int32_t nA;
    const double* vol_shocks;  /* host */ int32_t nV;
    double* net;       /* [B][8] */
    int32_t* n_dead;   /* [B] */
    double* pnl_ss; double* pnl_sm; /* [B][nA][nV], each may be NULL */
    int32_t* cell_flags;            /* [B][nA][nV] */
    int32_t cells_per_wg; /* 0 = chosen by the call; 1..256 = tuning / testing override, same bits */
} ivs_book_args;
int ivs_svi_book_f64(const ivs_book_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * P&L explain of a book between snapshots (rules X0-X9; additive to ABI 5).  Inputs as for
 * ivs_svi_book_f64 without the shocks, plus lag >= 1.  Pair p = 0 .. P-1, P = max(B - lag, 0), has end 0 = snapshot p and end 1 =
 * snapshot p + lag.  The contract is end 0's: K = spot[p] u[p][q] (strike_mode 0) or u[p][q] (1), used as an absolute strike at
 * end 1, whose u is not read; tau0 = tau[p][q], tau1 = tau[p+lag][q] (the same list with q_stride 0), dS = S1 - S0,
 * dt = tau0 - tau1.  Three placements by the rules of ivs_svi_eval_f64: (a) end 0 at (S0, K, tau0) with every Greek of
 * ivs_svi_greeks_f64 and the price P0, (b) end 1 at (S1, K, tau1) with the price P1 and the vol sigma1 = sqrt(W / tau1), (c) end
 * 0's slices at tau1, read at x = log(K/S0) - rate tau1 (sigma0_ss) and at x = log(K/S1) - rate tau1 (sigma0_sm).
 *
 * Per option, each [P][Q] and each may be NULL (then not written):
 *   actual                             P1 - P0
 *   theta_pnl                          theta dt
 *   delta_ss, gamma_ss, vega_ss        delta_ss dS, (gamma_ss / 2) dS^2, vega (sigma1 - sigma0_ss)
 *   resid_ss                           actual - (((theta_pnl + delta_ss) + gamma_ss) + vega_ss), in that order
 *   delta_sm, gamma_sm, vega_sm        the same from the sticky-moneyness Greeks and sigma0_sm
 *   resid_sm                           likewise
 * A product that is a zero of either sign is written as +0.0.
 *   flags [P][Q] (int32)               the IVS_SE_* bits of placement (a) in bits 0-7 (NEG_FWD included), of (b) in bits 8-15, of
 *                                      (c) in bits 16-23; required
 *   net [P][12]                        sum over the live options of qty x the ten figures above, in that order, then of
 *                                      qty P0 and of |qty| P0; required
 *   n_dead [P] (int32)                 required
 * An option is dead in a pair when any placement is dead or its quantity is not finite: NaN in its ten figures, nothing added to
 * net.  A pair with an UNORDERED end or an end without a live slice has NaN in every net entry and n_dead = Q.  The sums are
 * formed as in ivs_svi_book_f64 (no atomics, an order that depends on Q alone): the bits of a pair do not depend on B, on lag or on
 * the other pairs of the call.  A pair whose two ends carry the same bits in params, Tq, spot and tau has exactly +0.0 in the ten
 * figures of every live option and in net[0..9].
 *
 * IVS_EINVAL: null args or a null required pointer, a negative size, a stride that is neither 0 nor the full size, a
 * strike_mode that is not 0 or 1; IVS_ERANGE: mT > 64, lag < 1, B*mT or B*Q >= 2^31 (so P*Q < 2^31).  B <= lag, mT == 0 or Q == 0
 * is a no-op (nothing is written; engine.svi_explain defines the result); the limits above are checked before that.  A refused
 * call launches nothing.  No workspace, no allocation, no synchronisation (capturable); ONE launch.
 */
typedef struct ivs_explain_args {
    const double* params; /* [B][mT][5] */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* u; const double* tau; int64_t q_stride;
    const uint8_t* is_put; /* [Q] or NULL */
    const double* qty;     /* [Q] */
    int32_t strike_mode;
    int32_t mT; int64_t Q; int64_t B;
    int32_t lag;
    double* actual; double* theta_pnl; double* delta_ss; double* gamma_ss; double* vega_ss; double* resid_ss;
    double* delta_sm; double* gamma_sm; double* vega_sm; double* resid_sm; /* [P][Q], each may be NULL */
    double* net;       /* [P][12] */
    int32_t* n_dead;   /* [P] */
    int32_t* flags;    /* [P][Q] */
} ivs_explain_args;
int ivs_svi_explain_f64(const ivs_explain_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Historical-simulation value-at-risk and expected shortfall of a book per snapshot (rules H0-H9; additive
 * to ABI 5).  Inputs as for ivs_svi_explain_f64, plus window (scenarios kept per snapshot), nL tail probabilities (host array),
 * min_scen and scen_per_wg.  For snapshot p, scenario s = 0 .. window-1 is the past pair with start j = p - lag - s and end
 * j + lag; it exists while j >= 0.  The scenario moves today's spot by the pair's quotient, S' = S_p (S_{j+lag} / S_j), and every
 * live option's vol by the pair's change at the option's new moneyness x' = log(K / S') - rate tau and today's tau:
 * sigma' = sigma_p(x') + (sigma_{j+lag}(x') - sigma_j(x')), each sigma = sqrt(W(x') / tau) with that snapshot's own bracket and
 * weight by the rules of ivs_svi_eval_f64.  P' is the price formula of ivs_svi_greeks_f64 at (S', x', sigma' sqrt(tau)); the base
 * price P is the same code with the quotient 1.0 and the change +0.0.
 *   pnl [B][window]                    sum over the live options of qty (P' - P), formed as in ivs_svi_book_f64 (no atomics, an
 *                                      order that depends on Q alone): the bits of a scenario depend on snapshot p, the pair's two
 *                                      snapshots and the book alone.  NaN when the scenario has a flag.  Exactly +0.0 for a pair
 *                                      whose two ends carry the same bits in params, Tq and spot.  Required.
 *   scen_flags [B][window] (int32)     IVS_HS_ABSENT: j < 0; IVS_HS_VOID_PAIR: an end of the pair, or snapshot p itself, is
 *                                      UNORDERED or has no live slice (a spot that is not finite and > 0 leaves none); either
 *                                      is the scenario's only bit.  IVS_HS_NEG_VOL: a live option has !(sigma' > 0).  Required.
 *   n_valid [B] (int32)                the ranked scenarios: no flag and a P&L that is a number.  Required.
 *   var, es [B][nL]                    with n = n_valid, m = max(1, floor(n tp)) (one IEEE product): var = 0.0 - (the m-th smallest
 *                                      P&L), es = 0.0 - (the sum of the m smallest, added in rank order from +0.0, divided by m); ties
 *                                      rank by the lower s.  NaN when n < min_scen.  Required when nL > 0.
 *   worst [B] (int32)                  the s of the smallest P&L, -1 without a ranked scenario.  Required.
 *   n_dead [B] (int32)                 as in ivs_svi_book_f64.  Required.
 *   value [B][2]                       sum of qty P0 and of |qty| P0 over the live options, P0 the price of ivs_svi_greeks_f64;
 *                                      may be NULL.  NaN for an UNORDERED snapshot or one without a live slice (n_dead = Q).
 * scen_per_wg: how many scenarios one workgroup takes; 0 lets the call choose, 1..window forces it (the same bits).  stages: 0 =
 * both launches, 1 = the P&L kernel alone, 2 = the order statistics alone, read from pnl and scen_flags as given (measuring).
 *
 * IVS_EINVAL: null args or a null required pointer, a negative size, a stride that is neither 0 nor the full size, a
 * strike_mode that is not 0 or 1; IVS_ERANGE: mT > 64, lag < 1, window outside 1..1024, nL outside 0..8, a tail probability that
 * is not finite or not inside (0, 1), min_scen < 1, scen_per_wg outside 0..window, stages outside 0..2, B*mT, B*Q or B*window >=
 * 2^31.  B == 0, mT == 0 or Q == 0 is a no-op (nothing is written; engine.svi_hsim defines the result); the limits above are
 * checked before that.  B <= lag is not empty: every scenario is ABSENT.  A refused call launches nothing.  No workspace, no
 * allocation, no synchronisation (capturable); TWO launches.
 */
enum {
    IVS_HS_ABSENT = 1,
    IVS_HS_VOID_PAIR = 2,
    IVS_HS_NEG_VOL = 4
};
typedef struct ivs_hsim_args {
    const double* params; /* [B][mT][5] */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* u; const double* tau; int64_t q_stride;
    const uint8_t* is_put; /* [Q] or NULL */
    const double* qty;     /* [Q] */
    int32_t strike_mode;
    int32_t mT; int64_t Q; int64_t B;
    int32_t lag;
    int32_t window;            /* 1..1024 */
    const double* tail_probs;  /* host */ int32_t nL; /* 0..8 */
    int32_t min_scen;          /* >= 1 */
    int32_t scen_per_wg;       /* 0 = chosen by the call; 1..window = tuning / testing override, same bits */
    int32_t stages;            /* 0 = both; 1 = P&L only; 2 = order statistics only */
    double* pnl;           /* [B][window] */
    int32_t* scen_flags;   /* [B][window] */
    double* var; double* es; /* [B][nL] */
    int32_t* n_valid; int32_t* n_dead; int32_t* worst; /* [B] */
    double* value;         /* [B][2], may be NULL */
} ivs_hsim_args;
int ivs_svi_hsim_f64(const ivs_hsim_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Attribution of the VaR and expected shortfall of ivs_svi_hsim_f64 to the options of the book and to groups of them (DESIGN.md
 * section 20, rules A0-A8; additive to ABI 5): the Euler allocation of the tail.  Inputs as for ivs_svi_hsim_f64 without
 * scen_per_wg and stages, plus pnl and scen_flags [B][window] as an ivs_svi_hsim_f64 call on the same data wrote them (INPUTS
 * here), group [Q] (int32, device, one list for all snapshots; NULL = every option in group 0) and nG in 1..16.  An option
 * whose group id is outside 0..nG-1 is in no group.
 * Scenario s of snapshot p is ranked when it has no flag, its P&L is a number and it exists (s <= p - lag); the order is
 * ascending, ties by the lower s.  n = the ranked scenarios, m_l = max(1, floor(n tp_l)) (one IEEE product); level l is active
 * iff n >= min_scen and n > 0.  For rank r < max_l m_l with scenario s, t(q, r) = qty_q (P' - P) is the term of option q that
 * ivs_svi_hsim_f64 added to pnl[p][s]: the same device functions in the same order, the same bits.
 *   order [B][window] (int32)          the s of rank r for r < n, -1 after.  May be NULL.
 *   n_tail [B][nL] (int32)             m_l, 0 for an inactive level.  Required when nL > 0.
 *   ces [B][nL][Q]                     0.0 - (sum over r < m_l of t(q, r), added in rank order from +0.0) / m_l.  May be NULL.
 *   cvar [B][nL][Q]                    0.0 - t(q, m_l - 1).  May be NULL.
 *   cvar_group, ces_group [B][nL][nG]  the same with G(g, r) in place of t: the sum over the live options of group g of t(q, r),
 *                                      formed as ivs_svi_hsim_f64 forms a scenario's P&L (no atomics, an order that depends on
 *                                      Q alone).  With nG = 1 and group NULL they carry the bits of var and es.  Each may be NULL.
 * A dead option has NaN in ces and cvar; an inactive level and an UNORDERED snapshot or one without a live slice have NaN
 * everywhere; a group without a live member has +0.0.  An output left out is neither computed nor written.  Rows of pnl and
 * scen_flags that are not those of an ivs_svi_hsim_f64 call on the same data give unspecified values but no access out of range.
 *
 * IVS_EINVAL and IVS_ERANGE as for ivs_svi_hsim_f64, plus IVS_ERANGE: nG outside 1..16, and a level whose largest tail
 * max(1, floor(window tp_l)) exceeds 64 scenarios (the work grows with the tail and the per-rank group sums live in LDS; window
 * 1024 at 5 % is 51).  B == 0, mT == 0 or Q == 0 is a no-op (nothing is written; engine.svi_hsim_attrib defines the result);
 * the limits above are checked before that.  A refused call launches nothing and touches no buffer.  No workspace, no
 * allocation, no synchronisation (capturable); ONE launch.
 */
typedef struct ivs_hsim_attrib_args {
    const double* params; /* [B][mT][5] */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* u; const double* tau; int64_t q_stride;
    const uint8_t* is_put; /* [Q] or NULL */
    const double* qty;     /* [Q] */
    int32_t strike_mode;
    int32_t mT; int64_t Q; int64_t B;
    int32_t lag;
    int32_t window;            /* 1..1024 */
    const double* tail_probs;  /* host */ int32_t nL; /* 0..8 */
    int32_t min_scen;          /* >= 1 */
    const double* pnl;         /* [B][window], input */
    const int32_t* scen_flags; /* [B][window], input */
    const int32_t* group;      /* [Q] or NULL */
    int32_t nG;                /* 1..16 */
    double* ces; double* cvar;             /* [B][nL][Q], each may be NULL */
    double* ces_group; double* cvar_group; /* [B][nL][nG], each may be NULL */
    int32_t* n_tail;           /* [B][nL] */
    int32_t* order;            /* [B][window], may be NULL */
} ivs_hsim_attrib_args;
int ivs_svi_hsim_attrib_f64(const ivs_hsim_attrib_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Minimum-variance hedge of a book over its historical scenarios (rules M0-M11; additive to ABI 5): which of
 * nH candidate instruments, in which sizes, remove the most of the variance of the book's scenario P&L row, in at most `rounds`
 * steps of an orthogonal matching pursuit.  The book arrives as its row: pnl and scen_flags [B][window] as an ivs_svi_hsim_f64
 * call on the same data wrote them (INPUTS here).  The candidates are inst_u, inst_tau [nH] (inst_stride 0) or [B][nH]
 * (inst_stride nH), read as u and tau of ivs_svi_hsim_f64 under strike_mode, and inst_kind [nH] (uint8, device): 0 a call, 1 a put,
 * 2 the underlying (its u and tau are not read); any other value is read as a call.
 * Scenario s of snapshot p is ranked when it has no flag, its P&L is a number and it exists (s <= p - lag); n = the ranked
 * scenarios, and the snapshot is active iff n >= min_scen and n > 0.  Every sum below runs over the ranked scenarios in ascending s,
 * each product rounded, added serially from +0.0.
 *   inst_pnl [B][window][nH]           stage 1: the P&L x of one unit of candidate h in scenario s: P' - P as ivs_svi_hsim_f64 forms the
 *                                      term of an option at quantity 1.0 (the same bits), S' - S for the underlying; NaN when the
 *                                      scenario is absent or void, the candidate is dead at p or has !(sigma' > 0).  +0.0 for a pair
 *                                      whose ends carry the same bits.  Required; an INPUT of stage 2.
 *   inst_value [B][nH]                 stage 1: the base price P, S for the underlying, NaN for a dead candidate.  May be NULL.
 *   inst_flags [B][nH] (int32)         IVS_HG_DEAD: dead at p; IVS_HG_NEG_VOL: x is not a number in a ranked scenario; IVS_HG_FLAT:
 *                                      !(g > 0) with g = sum x^2; IVS_HG_SPENT: its g fell to tol x g or below after the picks before
 *                                      it (collinear with them), or its direction vanished.  A candidate with none of these is
 *                                      usable.  IVS_HG_CHOSEN: picked in some round (informative).
 *   pick [B][rounds] (int32)           the candidate of round k, -1 for an empty round.  Round k < n_forced takes candidate k when it
 *                                      is eligible (usable, not chosen, g_k > tol x g) and is empty otherwise; a later round takes the
 *                                      eligible candidate with the largest (a a) / g_k, a = sum x e on the current residual e, ties to
 *                                      the lower h, and when nobody is eligible or !(gain > min_gain x E_k) it and every later round
 *                                      are empty.
 *   ss [B][rounds+1]                   E_0 = sum pnl^2 and the residual sum of squares E_k after every round.
 *   n_rounds [B] (int32)               the rounds that are not empty.
 *   hedge [B][nH]                      the quantity to ADD to the book per candidate, +0.0 for one not picked.
 *   pnl_hedged [B][window]             pnl + sum over the picks in round order of hedge x inst_pnl, from pnl; NaN where not ranked.
 *   var_h, es_h [B][nL], worst_h,      ivs_svi_hsim_f64's var, es, worst and n_valid on (pnl_hedged, scen_flags); with every round empty
 *   n_scen [B] (int32)                 (an inactive snapshot included) they carry the bits of that call's own.
 *   solo_qty, solo_left [B][nH]        the hedge with candidate h alone, 0.0 - a / g, and the share (E_0 - (a a) / g) / E_0 of the
 *                                      variance it leaves; NaN for a candidate that is not usable.  Each may be NULL.
 * On an inactive snapshot pick is -1, n_rounds 0, ss, hedge and the solo figures NaN; inst_pnl, inst_flags bits 0-2 and pnl_hedged
 * (the row itself) stay as defined.  stages: 0 = everything, 1 = inst_pnl and inst_value alone, 2 = all but those, on inst_pnl as given.
 * scen_per_wg: as in ivs_svi_hsim_f64, for stage 1.
 *
 * IVS_EINVAL and IVS_ERANGE as for ivs_svi_hsim_attrib_f64 (nH in the place of Q, without nG and the cap on a level's tail), plus
 * IVS_ERANGE: nH > 64, rounds outside 1..8, n_forced outside 0..min(rounds, nH), tol not finite or outside [0, 1), min_gain not finite
 * or negative, stages outside 0..2, B*window*nH >= 2^31.  B == 0, mT == 0 or nH == 0 is a no-op (nothing is written); the limits are
 * checked before that.  A refused call launches nothing and touches no buffer.  No workspace, no allocation, no synchronisation
 * (capturable); up to THREE launches.  When (rounds + 1) x window x 8 bytes exceed 48 KB, the first call of a process at that
 * size (or a larger one than any before) also sets a function attribute of the selection kernel, which is no stream operation:
 * make such a call once outside a capture before capturing it.
 */
enum {
    IVS_HG_DEAD = 1,
    IVS_HG_NEG_VOL = 2,
    IVS_HG_FLAT = 4,
    IVS_HG_SPENT = 8,
    IVS_HG_CHOSEN = 16
};
typedef struct ivs_hedge_args {
    const double* params; /* [B][mT][5] */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* inst_u; const double* inst_tau; int64_t inst_stride;
    const uint8_t* inst_kind;  /* [nH] */
    int32_t strike_mode;
    int32_t mT; int32_t nH; /* 0..64 */ int64_t B;
    int32_t lag;
    int32_t window;            /* 1..1024 */
    const double* tail_probs;  /* host */ int32_t nL; /* 0..8 */
    int32_t min_scen;          /* >= 1 */
    int32_t rounds;            /* 1..8 */
    int32_t n_forced;          /* 0..min(rounds, nH) */
    double tol; double min_gain;
    int32_t stages;            /* 0 = all; 1 = inst_pnl only; 2 = selection and tail only */
    int32_t scen_per_wg;       /* 0 = chosen by the call; 1..window = tuning / testing override, same bits */
    const double* pnl;         /* [B][window], input */
    const int32_t* scen_flags; /* [B][window], input */
    double* inst_pnl;          /* [B][window][nH] */
    int32_t* inst_flags;       /* [B][nH] */
    int32_t* pick;             /* [B][rounds] */
    double* ss;                /* [B][rounds+1] */
    int32_t* n_rounds;         /* [B] */
    double* hedge;             /* [B][nH] */
    double* pnl_hedged;        /* [B][window] */
    double* var_h; double* es_h; /* [B][nL] */
    int32_t* worst_h; int32_t* n_scen; /* [B] */
    double* solo_qty; double* solo_left; double* inst_value; /* [B][nH], each may be NULL */
} ivs_hedge_args;
int ivs_svi_hedge_f64(const ivs_hedge_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * What-if VaR and expected shortfall of a book per candidate trade and size (rules W0-W9; additive to ABI 5):
 * what the tail figures of ivs_svi_hsim_f64 become when q units of candidate h are ADDED to the book, for every snapshot p, every
 * one of nH candidates and every one of nQ rungs of a ladder of sizes, in one launch.  The book arrives as its row (pnl, scen_flags
 * [B][window], INPUTS), the candidates as for ivs_svi_hedge_f64 (inst_u, inst_tau, inst_stride, inst_kind), the ladder as size
 * [nH][nQ] (size_stride 0) or [B][nH][nQ] (size_stride nH x nQ) on the device.  The ranked scenarios, n and "active" are those of
 * ivs_svi_hedge_f64.
 *   inst_pnl [B][window][nH]           stage 1: ivs_svi_hedge_f64's, by the same launch (the same bits).  Required; an INPUT of stage 2.
 *   inst_value [B][nH]                 stage 1: as there.  May be NULL.
 *   trade_flags [B][nH] (int32)        IVS_HG_NEG_VOL: x is not a number in a ranked scenario (a candidate dead at p is, whenever
 *                                      n > 0).  No other bit is set.
 *   var_w, es_w [B][nH][nQ][nL]        ivs_svi_hsim_f64's var and es of the row z_s = pnl_s + size x inst_pnl_s over the ranked
 *                                      scenarios (the product rounded, then the sum): ascending, ties to the lower s, m = max(1,
 *                                      floor(n x tp)), 0.0 - the m-th smallest and 0.0 - (the m smallest added serially from +0.0, / m).
 *   worst_w [B][nH][nQ] (int32)        the scenario of rank 0 of that row.  May be NULL.
 *                                      A rung is live iff its candidate has no flag, the snapshot is active, its size is finite and no
 *                                      z of its row is NaN (inf - inf, 0 x inf); one that is not has NaN, NaN and -1.
 *   best [B][nH][nL] (int32)           the live rung with the smallest es_w at that level (a NaN es_w never is), ties to the lower
 *                                      rung; -1 without one.
 *   var0, es0 [B][nL], worst0,         ivs_svi_hsim_f64's var, es, worst and n_valid of the row itself, formed here: the bits of that
 *   n_scen [B] (int32)                 call's own on the same inputs.
 * stages: 0 = everything, 1 = inst_pnl and inst_value alone, 2 = all but those, on inst_pnl as given.  scen_per_wg: for stage 1.
 *
 * IVS_EINVAL and IVS_ERANGE as for ivs_svi_hedge_f64 (without rounds, n_forced, tol and min_gain), plus IVS_ERANGE: nQ outside 1..16,
 * B*nH*nQ*max(nL,1) >= 2^31; IVS_EINVAL: a size_stride that is neither 0 nor nH x nQ.  B == 0, mT == 0 or nH == 0 is a no-op (nothing
 * is written); the limits are checked before that.  A refused call launches nothing and touches no buffer.  No workspace, no
 * allocation, no synchronisation (capturable), no dynamic LDS; at most TWO launches.
 */
typedef struct ivs_whatif_args {
    const double* params; /* [B][mT][5] */
    const double* Tq; int64_t tq_stride;
    const double* spot; double rate;
    const double* inst_u; const double* inst_tau; int64_t inst_stride;
    const uint8_t* inst_kind;  /* [nH] */
    int32_t strike_mode;
    int32_t mT; int32_t nH; /* 0..64 */ int64_t B;
    int32_t lag;
    int32_t window;            /* 1..1024 */
    const double* tail_probs;  /* host */ int32_t nL; /* 0..8 */
    int32_t min_scen;          /* >= 1 */
    int32_t nQ;                /* 1..16 */
    const double* size; int64_t size_stride; /* [nH][nQ] (0) or [B][nH][nQ] (nH * nQ), device */
    int32_t stages;            /* 0 = all; 1 = inst_pnl only; 2 = the ladder only */
    int32_t scen_per_wg;       /* 0 = chosen by the call; 1..window = tuning / testing override, same bits */
    const double* pnl;         /* [B][window], input */
    const int32_t* scen_flags; /* [B][window], input */
    double* inst_pnl;          /* [B][window][nH] */
    double* inst_value;        /* [B][nH], may be NULL */
    int32_t* trade_flags;      /* [B][nH] */
    double* var_w; double* es_w; /* [B][nH][nQ][nL] */
    int32_t* worst_w;          /* [B][nH][nQ], may be NULL */
    int32_t* best;             /* [B][nH][nL] */
    double* var0; double* es0; /* [B][nL] */
    int32_t* worst0; int32_t* n_scen; /* [B] */
} ivs_whatif_args;
int ivs_svi_whatif_f64(const ivs_whatif_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Bootstrap standard errors and intervals for a book's VaR and expected shortfall (rules C0-C9; additive to
 * ABI 5): how far the tail figures of ivs_svi_hsim_f64 move when the row of scenario P&Ls is resampled.  The call works on rows
 * alone: pnl and scen_flags [B][window] as an ivs_svi_hsim_f64 call wrote them (INPUTS; any rows with that meaning, the hedged row of
 * ivs_svi_hedge_f64 for one); no slices, no book, no lag.  The ranked scenarios, their order (ascending, ties to the lower s) and n
 * are ivs_svi_hsim_f64's; the ranked scenarios in ascending s are the time positions 0..n-1.  A row is active iff n >= min_scen,
 * n > 0 and every ranked value is finite.  Replicate r of n_rep is a circular block bootstrap: ceil(n / L') blocks of L' = min(block, n)
 * consecutive positions (mod n), each starting at (u n) >> 32 for the upper word u of a splitmix64 finaliser at the counter
 * (r << 32 | block index) and `seed`, laid end to end and cut at n draws.  A replicate's VaR and ES are ivs_svi_hsim_f64's on the
 * drawn values: m = max(1, floor(n x tp)); up the ranks, each drawn rank adds (double)k x v with k = min(its count, what is left of m),
 * serially from +0.0; 0.0 - the value at which m is reached and 0.0 - sum / m.
 *   var0, es0 [B][nL], n_scen [B] (int32)   ivs_svi_hsim_f64's var, es and n_valid of the row itself, formed here (the same bits).
 *   mean, variance [B][2][nL]               over the n_rep replicate values of statistic 0 = VaR, 1 = ES at every level: the sum in the
 *                                           order of rule B5 over the replicates (passes of 256) / n_rep, and the sum of the rounded
 *                                           squares of (value - mean) in the same order / (n_rep - 1) (NaN for n_rep = 1).
 *   quant [B][2][nL][nC]                    the i-th smallest (from 0) of the replicate values, i = min(n_rep - 1, floor(n_rep x ci)).
 *   rep [B][n_rep][2][nL]                   the replicate values themselves.  May be NULL; the call then keeps them in the workspace.
 * A row that is not active has NaN in mean, variance, quant and rep.  The bits of a row's outputs depend on the row, tail_probs,
 * min_scen, block, seed, ci_probs and n_rep alone, and rep[p][r] on n_rep only through r < n_rep.
 *
 * workspace: ivs_hsim_bootstrap_workspace_bytes(B, n_rep, nL) bytes of device memory, 8-byte aligned, when rep is NULL; with rep given
 * none is needed (NULL, 0).  That function returns 0 for sizes the call refuses.
 * IVS_EINVAL: null args, a negative size, a null required pointer (tail_probs with nL > 0, ci_probs with nC > 0, pnl, scen_flags,
 * n_scen, and with nL > 0 var0, es0, mean, variance, with nC > 0 also quant), a workspace that is missing or too small.  IVS_ERANGE:
 * window outside 1..1024, nL > 8, a tail probability outside (0, 1), min_scen < 1, n_rep or block outside 1..1024, nC > 8, an
 * interval probability that is not finite and inside (0, 1), B*window, B*n_rep*2*max(nL,1) or B*2*max(nL,1)*max(nC,1) >= 2^31.  The
 * limits are checked before the zero-size return; B == 0 is a no-op.  A refused call launches nothing and touches no buffer.  No
 * allocation, no synchronisation (capturable), no dynamic LDS; ONE launch.
 */
typedef struct ivs_bootstrap_args {
    const double* pnl;         /* [B][window], input */
    const int32_t* scen_flags; /* [B][window], input */
    int64_t B;
    int32_t window;            /* 1..1024 */
    int32_t nL;                /* 0..8 */
    const double* tail_probs;  /* host */
    int32_t min_scen;          /* >= 1 */
    int32_t n_rep;             /* 1..1024 */
    int32_t block;             /* 1..1024 */
    int32_t nC;                /* 0..8 */
    uint64_t seed;
    const double* ci_probs;    /* host, each inside (0, 1) */
    double* var0; double* es0; /* [B][nL] */
    int32_t* n_scen;           /* [B] */
    double* mean; double* variance; /* [B][2][nL] */
    double* quant;             /* [B][2][nL][nC] */
    double* rep;               /* [B][n_rep][2][nL], may be NULL */
} ivs_bootstrap_args;
size_t ivs_hsim_bootstrap_workspace_bytes(int64_t B, int32_t n_rep, int32_t nL);
int ivs_hsim_bootstrap_f64(const ivs_bootstrap_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Age-weighted, volatility-scaled historical-simulation VaR and expected shortfall (rules W0-W9; additive to
 * ABI 5).  The call works on rows: pnl and scen_flags [B][window] as an ivs_svi_hsim_f64 call wrote them (INPUTS), with the lag of
 * that call, and on the snapshots' spot [B] when scaling is on (vol_span = M > 0).  Scenario s of a row has the weight weight[s] (by
 * its age; NULL: every weight 1.0).  With M > 0 a running vol of the spot is formed first: r_j = spot[j] / spot[j-1] - 1.0 (valid iff
 * both spots are finite and > 0 and r_j is finite), sigma[j] = sqrt(sum_k a_k (r_{j-k} r_{j-k}) / sum_k a_k) over k = 0..M-1 in
 * ascending k from +0.0, a_k = vol_weight[k], terms with j - k < 1 or an invalid return left out of both sums; NaN with fewer than
 * min_returns terms, with an a_k among them that is not finite and >= 0, or with a quotient that is not finite and > 0.  Scenario s of
 * snapshot p starts at j = p - lag - s; it is multiplied by f = min(max(sigma[p] / sigma[j], 1 / scale_cap), scale_cap): z = pnl f.
 * With M == 0 z is pnl to the bit and neither sigma nor spot is read.
 *   flags_w [B][window] (int32)        scen_flags | IVS_HW_NO_VOL (M > 0 and j < 0, or either sigma not finite and > 0) |
 *                                      IVS_HW_BAD_WEIGHT (weight[s] not finite and >= 0).  Required.
 *   n_valid_w, worst_w [B] (int32)     the ranked scenarios (flags_w == 0 and z a number), and the s of the smallest z (ties to the
 *                                      lower s, -0.0 == +0.0; -1 without one).  Required.
 *   wsum, n_eff [B]                    W = the sum of the ranked scenarios' weights, in the order of rule B5 over s (passes of 256), and
 *                                      (W W) / W2 with W2 the sum of the rounded squares in that order (NaN when W2 is not > 0).  Required.
 *   var_w, es_w [B][nL]                the weighted tail at every level: target = tp W; up the ranks in ascending z the weights are
 *                                      added until the next one would reach the target; 0.0 - z at that rank, and 0.0 - (the sum of the
 *                                      rounded w z below it + (target - the weight below it) z at it) / target: the exact tail mean,
 *                                      with a fractional share of the boundary scenario.  NaN unless n >= min_scen, n > 0 and W is
 *                                      finite and > 0.
 *   pnl_w, scale [B][window]           z (NaN where the scenario is not ranked) and f (NaN where none was formed, 1.0 with M == 0).
 *                                      Either may be NULL.  pnl_w with flags_w is a row in ivs_svi_hsim_f64's sense.
 *   sigma [B]                          output at stages 0 and 1, INPUT at stages 2; required iff M > 0.
 * stages: 0 = both launches, 1 = sigma alone, 2 = the tail alone on sigma as given.  With M == 0, stages 1 has nothing to do.
 * The bits of a row's outputs depend on the row, the sigmas it reads, weight, tail_probs, min_scen and the settings alone.
 *
 * No workspace (NULL, 0).  IVS_EINVAL: null args, a negative size (B, nL), a null required pointer (tail_probs with nL > 0; at
 * stages 0 and 2 pnl, scen_flags, flags_w, n_valid_w, worst_w, wsum, n_eff, and with nL > 0 var_w, es_w; with M > 0 sigma, and at
 * stages 0 and 1 also spot and vol_weight).  IVS_ERANGE: lag < 1, window outside 1..1024, nL > 8, a tail probability outside (0, 1),
 * min_scen < 1, vol_span outside 0..1024, with M > 0 min_returns outside 1..M or scale_cap not finite or < 1, stages outside 0..2,
 * B*window >= 2^31.  The limits are checked before the zero-size return; B == 0 is a no-op.  A refused call launches nothing and
 * touches no buffer.  No allocation, no synchronisation (capturable), no dynamic LDS; at most two launches, one when M == 0 or
 * stages != 0.
 */
enum {
    IVS_HW_NO_VOL = 8,
    IVS_HW_BAD_WEIGHT = 16
};
typedef struct ivs_hsim_weighted_args {
    const double* pnl;         /* [B][window], input */
    const int32_t* scen_flags; /* [B][window], input */
    int64_t B;
    int32_t window;            /* 1..1024 */
    int32_t lag;               /* >= 1 */
    int32_t nL;                /* 0..8 */
    int32_t min_scen;          /* >= 1 */
    const double* tail_probs;  /* host */
    const double* weight;      /* [window] by age, may be NULL: 1.0 */
    const double* spot;        /* [B], with vol_span > 0 */
    const double* vol_weight;  /* [vol_span], with vol_span > 0 */
    int32_t vol_span;          /* 0..1024; 0 = no scaling */
    int32_t min_returns;       /* 1..vol_span */
    double scale_cap;          /* finite, >= 1 */
    int32_t stages;            /* 0..2 */
    double* sigma;             /* [B], with vol_span > 0 */
    double* var_w; double* es_w; /* [B][nL] */
    int32_t* n_valid_w; int32_t* worst_w; /* [B] */
    double* wsum; double* n_eff; /* [B] */
    double* pnl_w; double* scale; /* [B][window], may be NULL */
    int32_t* flags_w;          /* [B][window] */
} ivs_hsim_weighted_args;
int ivs_hsim_weighted_f64(const ivs_hsim_weighted_args* args /* host */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Black-Scholes Greeks epilogue (reference src/interpolation/greeks.py:12-43, BlackScholesGreeks.calculate_greeks):
 * elementwise over n options.  is_put [n] (1 = put) or NULL -> every option uses default_is_put.
 * theta is per day (/365), vega and rho per 1 % (/100), put rho without sign flip -- all as the reference.
 */
int ivs_bs_greeks_f64(const double* S, const double* K, const double* T, const double* r, const double* sigma,
                      const uint8_t* is_put, int32_t default_is_put, int64_t n, double* delta, double* gamma,
                      double* theta, double* vega, double* rho, void* stream);

/*
 * Black-Scholes prices and their inverse, price -> implied volatility (rules V1-V8): elementwise over n
 * options, one launch per call.  is_put [n] (1 = put) or NULL -> every option uses default_is_put.  With D = exp(-r T),
 * KD = K D and x = log(S/K) + r T:
 *
 * ivs_bs_price_f64: call = S Phi(d1) - KD Phi(d2), put = KD Phi(-d2) - S Phi(-d1), d1 = x/s + s/2, d2 = d1 - s,
 * s = sigma sqrt(T).  An option is live iff S, K, T, r, sigma are finite and S, K, T, sigma > 0; otherwise NaN and IVS_IV_DEAD.
 *   price [n]                          required
 *   vega [n]                           S phi(d1) sqrt(T), per unit of vol (NOT per 1 % like ivs_bs_greeks_f64); may be NULL
 *   flags [n] (int32)                  IVS_IV_DEAD or 0; may be NULL.  An output left out is neither computed nor written.
 *
 * ivs_bs_implied_vol_f64: the vol at which the formula above gives `price`.  price_mode 0: P = price; 1: P = price S (a
 * price quoted in units of the underlying, as the chains' mark_price is).  An option is live iff price, S, K, T, r are
 * finite, S, K, T > 0 and price >= 0; otherwise NaN and IVS_IV_DEAD alone.  The bounds are compared in price space:
 * P >= S (call) or KD (put) is IVS_IV_ABOVE (NaN); P below the intrinsic value max(S - KD, 0) / max(KD - S, 0) is
 * IVS_IV_BELOW (NaN), P equal to it IVS_IV_BELOW with vol 0.  An in-the-money option (call with x > 0, put with x < 0) carries
 * IVS_IV_ITM and is solved through parity on its time value P - intrinsic.  The total vol s solves
 * exp(-h/2) Phi(-h/s + s/2) - exp(h/2) Phi(-h/s - s/2) = tv / sqrt(S KD), h = |x|, by 64 halvings of log2 s on [-40, 6] in
 * every lane; a solution outside [2^-40, 2^6] gives that border and IVS_IV_EDGE.  vol = s / sqrt(T).
 *   vol [n], flags [n] (int32)         both required
 *
 * IVS_EINVAL: a null required pointer, n < 0, a price_mode that is not 0 or 1; IVS_ERANGE: n >= 2^31; n == 0 is a no-op.  A
 * refused call launches nothing.  No workspace, no allocation, no synchronisation (capturable).  The results do not depend on
 * n, on the option's position or on the launch geometry, bit for bit.
 */
enum {
    IVS_IV_ITM        = 1,
    IVS_IV_BELOW      = 2,
    IVS_IV_ABOVE      = 4,
    IVS_IV_DEAD       = 8,
    IVS_IV_EDGE       = 16
};
int ivs_bs_price_f64(const double* S, const double* K, const double* T, const double* r, const double* sigma,
                     const uint8_t* is_put, int32_t default_is_put, int64_t n,
                     double* price, double* vega /* may be NULL */, int32_t* flags /* may be NULL */, void* stream);
int ivs_bs_implied_vol_f64(const double* price, const double* S, const double* K, const double* T, const double* r,
                           const uint8_t* is_put, int32_t default_is_put, int32_t price_mode, int64_t n,
                           double* vol, int32_t* flags, void* stream);

/*
 * N-minute candle aggregation (reference src/candle_reconstruction/core.py:68-88) for S symbols (CSR series_off [S+1],
 * rows sorted by timestamp within a symbol).  For every input row i: if it is the first row of its
 * floor(ts / freq_ns) bucket, out_*[i] holds the bucket's candle (open = first non-NaN, high = max, low = min,
 * close = last non-NaN, volume = Kahan sum in row order, like pandas) and out_count[i] its row count; otherwise
 * out_count[i] = 0.  The caller keeps the rows with out_count >= N (incomplete groups are dropped, core.py:86-88).
 */
int ivs_candle_aggregate_f64(const int64_t* ts_ns, const double* open, const double* high, const double* low,
                             const double* close, const double* volume, const int64_t* series_off, int64_t n_series,
                             int64_t n_rows, int64_t freq_ns, int64_t* out_ts, double* out_open, double* out_high,
                             double* out_low, double* out_close, double* out_volume, int32_t* out_count, void* stream);

/*
 * IV -> OHLCV bridge (reference src/data_bridge/ohlcv_converter.py:138-369, InterpolatedToOHLCVConverter.
 * _generate_ohlcv_from_interpolated and its four candle builders).  The reference draws from NumPy's process-global
 * legacy generator; its numbers are reproduced by consuming the SAME MT19937 stream in the same order.
 *
 * ivs_mt19937_words_u32: the first n_words raw 32-bit outputs of np.random.seed(seed) into words (device).
 *
 * ivs_bridge_candles_f64: S symbols (CSR row_off [S+1]) over total_rows interpolated rows, processed in row order like
 * the reference's sequential loops.  price [total_rows] = the selected price column, volume [total_rows] or NULL
 * (column absent).  strategy: 0 spread_simulation (:209-263; base_spread_pct / vol_factor = its spread_parameters),
 * 1 price_as_midpoint (:265-290), 2 trend_following (:292-332), 3 simple_spread (:334-357, also the reference's
 * fallback for unknown names), 4 the inline variant of CompleteOptimizedPipeline._generate_ohlcv_candles (reference
 * complete_pipeline.py:473-510; price = its per-row `underlying or mark or index` choice, made by the caller).  words [n_words]: the stream positioned at this call's first draw.
 * out [6][total_rows]: open, high, low, close (Python round(x, 4)), volume (round(x, 6)), source_price; rows the
 * reference skips (price NaN or <= 0, :156-157) get valid = 0 and NaN.  rng_tail (device int64[4]):
 * [0] out: words consumed; [1],[2] in/out: the legacy generator's cached normal deviate (has_gauss, gauss bits; pass
 * zeros after a fresh seed); [3] out: 1 if n_words was too small (results invalid: regenerate more words and retry).
 * workspace: ivs_bridge_workspace_bytes(total_rows) bytes of device scratch.
 */
size_t  ivs_bridge_workspace_bytes(int64_t total_rows);
int     ivs_mt19937_words_u32(uint32_t seed, uint32_t* words, int64_t n_words, void* stream);
int     ivs_bridge_candles_f64(const double* price, const double* volume, const int64_t* row_off, int64_t S,
                               int64_t total_rows, int32_t strategy, double base_spread_pct, double vol_factor,
                               const uint32_t* words, int64_t n_words, double* out, uint8_t* valid, int64_t* rng_tail,
                               void* workspace, size_t workspace_bytes, void* stream);

/* name of the kernel the last ivs_surface_batch_f64 / ivs_snapshot_assemble_f64 / ivs_smile_delta_points_f64 /
 * ivs_surface_arbitrage_f64 / ivs_surface_moments_f64 / ivs_svi_slices_f64 / ivs_svi_distribution_f64 call on this thread
 * dispatched to (host string); ivs_svi_calendar_f64, ivs_svi_eval_f64, ivs_ssvi_surface_f64, ivs_bs_price_f64,
 * ivs_bs_implied_vol_f64, ivs_svi_greeks_f64, ivs_svi_book_f64, ivs_svi_explain_f64, ivs_svi_hsim_f64, ivs_svi_hsim_attrib_f64, ivs_svi_hedge_f64,
 * ivs_svi_whatif_f64, ivs_hsim_bootstrap_f64 and ivs_hsim_weighted_f64 set it too */
const char* ivs_last_kernel(void);

/*
 * Diagnostics (not part of the drop-in surface).  ivs_debug_stamps(buf, n): while `buf` (device,
 * n uint64, n >= 8 * 8 * CU count) is set, ivs_surface_batch_f64 runs the STAMPED build of the dense
 * kernel, which sums s_memtime deltas per phase and per workgroup into buf[wg*8 + phase]
 * (phase 7 = surfaces processed).  Pass NULL to return to the production kernel.  Returns the
 * number of slots per workgroup.  Stamped runs are for phase SHARES only, never for timing claims.
 */
int     ivs_debug_stamps(void* device_buf, int64_t n_u64);
int64_t ivs_debug_last_grid(void);   /* workgroups of the last dense launch */
/* byte offset, in the workspace a 64 x 16 surface call was given, of the int32 'missing quotes first' flag that call's
 * probe left there (1 = the compaction kernel took every surface); tests read it back after the call */
int64_t ivs_debug_mode_offset(void);

#ifdef __cplusplus
}
#endif
#endif /* IVS_H */
