"""Black-Scholes prices and price -> implied volatility on the MI355X engine (the inverse the
reference's ``src/interpolation/greeks.py`` leaves to whoever computed its ``iv`` column).  Scalars / NumPy arrays in ->
NumPy out (one H2D/D2H round trip); torch CUDA tensors in -> tensors out, the way greeks.BlackScholesGreeks does."""
import numpy as np

from . import _lib, engine

PRICE_MODES = engine.PRICE_MODES          # "quote": price in the units of S and K; "underlying": price x S (mark_price)
FLAG_NAMES = (("itm", _lib.IV_ITM), ("below", _lib.IV_BELOW), ("above", _lib.IV_ABOVE), ("dead", _lib.IV_DEAD), ("edge", _lib.IV_EDGE))


def price_mode_code(price_mode) -> int:
    """0 / 1 of the C ABI for "quote" / "underlying" (or 0 / 1 themselves); ValueError otherwise."""
    if isinstance(price_mode, str) and price_mode in PRICE_MODES:
        return PRICE_MODES[price_mode]
    if not isinstance(price_mode, (str, bool)) and price_mode in (0, 1):
        return int(price_mode)
    raise ValueError(f"price_mode {price_mode!r} is neither 'quote' nor 'underlying'")


def is_put_of(option_type) -> bool:
    if option_type in ("call", "c", "C"):
        return False
    if option_type in ("put", "p", "P"):
        return True
    raise ValueError(f"option_type {option_type!r} is neither 'call' nor 'put'")


class HipImpliedBackend:
    """Host arrays (flat float64, is_put uint8 or None) -> host arrays through the device kernels."""

    def __init__(self, stream=None):
        self.stream = stream

    def _dev(self, arrays, is_put):
        torch = engine.require_device()
        dev = [torch.from_numpy(np.ascontiguousarray(a, np.float64)).cuda() for a in arrays]
        put = None if is_put is None else torch.from_numpy(np.ascontiguousarray(is_put, np.uint8)).cuda()
        return dev, put

    def price(self, S, K, T, r, sigma, is_put, default_is_put=False):
        dev, put = self._dev((S, K, T, r, sigma), is_put)
        out = engine.bs_price(*dev, is_put=put, default_is_put=default_is_put, want_vega=True, stream=self.stream)
        return {k: v.cpu().numpy() for k, v in out.items()}

    def implied_vol(self, price, S, K, T, r, is_put, default_is_put=False, price_mode=0):
        dev, put = self._dev((price, S, K, T, r), is_put)
        out = engine.bs_implied_vol(*dev, is_put=put, default_is_put=default_is_put, price_mode=price_mode, stream=self.stream)
        return {k: v.cpu().numpy() for k, v in out.items()}


def _on_device(args):
    return all(hasattr(a, "is_cuda") and a.is_cuda for a in args)


def _host(args):
    """Scalars / arrays broadcast to one shape: (flat float64 arrays, shape)."""
    arrs = np.broadcast_arrays(*[np.asarray(a, np.float64) for a in args])
    return [np.ascontiguousarray(a).ravel() for a in arrs], arrs[0].shape


def _shaped(res, shape):
    res = {k: v.reshape(shape) for k, v in res.items()}
    return {k: v[()] for k, v in res.items()} if shape == () else res


class ImpliedVolatility:
    @staticmethod
    def price(S, K, T, r, sigma, option_type="call", backend=None):
        """dict(price, vega, flags): the Black-Scholes price of every option, its vega per unit of vol, and IV_DEAD where an
        input is not finite or not positive (then NaN)."""
        put = is_put_of(option_type)
        args = (S, K, T, r, sigma)
        if backend is None and _on_device(args):
            return engine.bs_price(*args, default_is_put=put, want_vega=True)
        flat, shape = _host(args)
        return _shaped((backend or HipImpliedBackend()).price(*flat, None, default_is_put=put), shape)

    @staticmethod
    def implied_vol(price, S, K, T, r, option_type="call", price_mode="quote", backend=None):
        """dict(vol, flags): the vol at which Black-Scholes gives `price`, and the _lib.IV_* bits.  price_mode "quote": the
        price is in the units of S and K; "underlying": it is quoted in units of the underlying (price x S, the convention of
        the chains' mark_price)."""
        put, mode = is_put_of(option_type), price_mode_code(price_mode)
        args = (price, S, K, T, r)
        if backend is None and _on_device(args):
            return engine.bs_implied_vol(*args, default_is_put=put, price_mode=mode)
        flat, shape = _host(args)
        return _shaped((backend or HipImpliedBackend()).implied_vol(*flat, None, default_is_put=put, price_mode=mode), shape)


def count_flags(flags) -> dict:
    """Rows per flag of a solver result: {"solved_rows", "itm_rows", "below_rows", "above_rows", "dead_rows", "edge_rows"}."""
    f = np.asarray(flags).astype(np.int64)
    out = {"solved_rows": int(((f & (_lib.IV_BELOW | _lib.IV_ABOVE | _lib.IV_DEAD | _lib.IV_EDGE)) == 0).sum())}
    out.update({f"{name}_rows": int(((f & bit) != 0).sum()) for name, bit in FLAG_NAMES})
    return out
