"""An e4m3 (OCP e4m3fn: 4 exponent bits, bias 7, 3 mantissa bits, no infinities, largest finite value 448) rounding that is not
the cast under test: the 127 non-negative finite values are written down from the format's definition and a value is rounded by
looking up its two neighbours in that table, in f64.  Nothing here goes through ``.to(torch.float8_e4m3fn)``.  Both functions
compute on the device their argument lives on (plain torch integer / f64 ops), so a GPU test does not move its tensors."""
import torch

E4M3_MAX = 448.0
NAN_CODE = 0x7F   # with either sign bit: 0x7f / 0xff


def _table():
    vals = []
    for code in range(127):            # 0x00 .. 0x7e; 0x7f is NaN
        e, m = code >> 3, code & 7
        vals.append(m * 2.0 ** -9 if e == 0 else (1 + m / 8) * 2.0 ** (e - 7))
    return torch.tensor(vals, dtype=torch.float64)


TABLE = _table()


def e4m3_values(codes):
    """uint8 codes -> f64 values (0x7f / 0xff -> NaN)."""
    c = codes.detach().contiguous().view(torch.uint8).to(torch.int64)
    mag = c & 0x7F
    v = TABLE.to(c.device)[mag.clamp(max=126)]
    v = torch.where(mag == NAN_CODE, torch.full_like(v, float("nan")), v)
    return torch.where((c & 0x80) != 0, -v, v)


def e4m3_codes(x):
    """The uint8 code of the e4m3fn value nearest to clamp(x, +-448): ties to the even code, the sign bit kept (-0.0 -> 0x80,
    a value that rounds to zero keeps its sign), +-inf saturated, NaN -> 0x7f | sign."""
    x = x.detach().to(torch.float64)
    table = TABLE.to(x.device)
    sign = torch.signbit(x).to(torch.int64) << 7
    a = x.abs().clamp(max=E4M3_MAX)
    nan = torch.isnan(a)
    a = torch.where(nan, torch.zeros_like(a), a)
    hi = torch.bucketize(a, table).clamp(max=126)        # first code whose value is >= a
    lo = (hi - 1).clamp(min=0)
    d_lo, d_hi = a - table[lo], table[hi] - a            # both exact in f64 wherever they can be equal
    take_hi = (d_hi < d_lo) | ((d_hi == d_lo) & (hi % 2 == 0))
    mag = torch.where(take_hi, hi, lo)
    mag = torch.where(nan, torch.full_like(mag, NAN_CODE), mag)
    return (mag | sign).to(torch.uint8)
