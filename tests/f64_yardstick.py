"""The float64 yardstick of the exact-arithmetic tests (a plain helper module, not a conftest).

A kernel result is held to a float64 statement of the same operation, with the same statement run in fp32 (torch or
numpy on the CPU) as the measure of what fp32 arithmetic costs.  Per tensor: RMS error <= RMS_K x the fp32 RMS error
and largest error <= MAX_K x the fp32 largest error, each + ULPS units in the last place of the tensor's scale.  Two
fp32 implementations that sum in different orders make independent roundoff of the same size; over the few hundred
to few hundred thousand entries of a tensor their RMS errors agree to well under 2x and their maxima (a tail
statistic) to under 4x, and the factors allow 2x on top.
"""
import numpy as np

RMS_K, MAX_K, ULPS = 4.0, 8.0, 8.0
ULP = 2.0 ** -24


def gap(got, want64, ref32, scale=None):
    """(ok, report) of a kernel result and the fp32 CPU result against the float64 value."""
    want = np.asarray(want64, np.float64)
    e = np.asarray(got, np.float64) - want
    e32 = np.asarray(ref32, np.float64) - want
    scale = float(np.abs(want).max()) if scale is None else float(scale)
    floor = ULPS * ULP * scale
    rms, rms32 = float(np.sqrt(np.mean(e * e))), float(np.sqrt(np.mean(e32 * e32)))
    mx, mx32 = float(np.abs(e).max()), float(np.abs(e32).max())
    ok = bool(np.isfinite(e).all()) and rms <= RMS_K * rms32 + floor and mx <= MAX_K * mx32 + floor
    return ok, dict(rms=rms, rms32=rms32, max=mx, max32=mx32, scale=scale)
