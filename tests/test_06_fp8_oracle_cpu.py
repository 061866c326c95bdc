"""tests/fp8_oracle.py against torch's CPU cast: the table-based e4m3 rounding the fp8 kernel tests use as their reference must
agree, code for code, with ``x.clamp(-448, 448).to(torch.float8_e4m3fn)`` -- on random values of every magnitude the format
resolves and on the values where a rounding goes wrong first (zeros, the subnormal step, ties, the saturation bound)."""
import torch

import fp8_oracle

FP8 = torch.float8_e4m3fn


def _torch_codes(x):
    return x.clamp(-448, 448).to(FP8).view(torch.uint8)


def test_table_is_the_format():
    t = fp8_oracle.TABLE
    assert t.numel() == 127 and t[0] == 0 and t[1] == 2.0 ** -9 and t[8] == 2.0 ** -6 and t[0x38] == 1.0 and t[126] == 448.0
    assert (t[1:] > t[:-1]).all()
    # every finite code decodes to what torch decodes it to, both signs; the NaN codes decode to NaN
    codes = torch.arange(256, dtype=torch.uint8)
    want = codes.view(FP8).double()
    got = fp8_oracle.e4m3_values(codes)
    finite = (codes & 0x7F) != 0x7F
    assert torch.equal(got[finite], want[finite]) and torch.equal(torch.signbit(got[finite]), torch.signbit(want[finite]))
    assert torch.isnan(got[~finite]).all() and torch.isnan(want[~finite]).all()
    # and encodes back to itself
    assert torch.equal(fp8_oracle.e4m3_codes(got[finite]), codes[finite])


def test_codes_match_torch_cpu_cast_on_random_values():
    g = torch.Generator().manual_seed(0)
    parts = [torch.randn(300_000, generator=g) * s for s in (1.0, 30.0, 0.01)]
    # log-uniform magnitudes from below the smallest subnormal to above the bound, both signs
    mag = torch.exp2(torch.rand(200_000, generator=g) * 24 - 14)
    parts.append(mag * (torch.randint(0, 2, (200_000,), generator=g) * 2 - 1))
    x = torch.cat(parts)
    assert x.numel() == 1_100_000
    got, want = fp8_oracle.e4m3_codes(x), _torch_codes(x)
    assert torch.equal(got, want), (x[got != want][:8], got[got != want][:8], want[got != want][:8])
    assert torch.equal(fp8_oracle.e4m3_codes(x.double()), want)


def test_codes_match_torch_cpu_cast_on_the_edges():
    s = 2.0 ** -9
    inf = float("inf")
    edges = [0.0, -0.0, s / 2, -s / 2, s, -s, 1.5 * s, -1.5 * s, 2.5 * s, -2.5 * s, 448.0, -448.0, 464.0, -464.0, 465.0, -465.0,
             1e9, -1e9, inf, -inf]
    # every midpoint between neighbouring codes (a tie), and the f32 values just beside it
    t = fp8_oracle.TABLE
    mid = ((t[1:] + t[:-1]) / 2).float()
    assert torch.equal(mid.double(), (t[1:] + t[:-1]) / 2)        # the midpoints are exact in f32
    x = torch.cat([torch.tensor(edges), mid, -mid, torch.nextafter(mid, torch.zeros(())), torch.nextafter(mid, torch.full((), inf))])
    got, want = fp8_oracle.e4m3_codes(x), _torch_codes(x)
    assert torch.equal(got, want), (x[got != want], got[got != want], want[got != want])
    named = dict(zip(edges, fp8_oracle.e4m3_codes(torch.tensor(edges)).tolist()))
    assert fp8_oracle.e4m3_codes(torch.tensor([0.0, -0.0])).tolist() == [0x00, 0x80]
    assert named[s / 2] == 0x00 and named[-s / 2] == 0x80            # the tie at half the smallest subnormal goes to even: zero
    assert named[s] == 0x01 and named[1.5 * s] == 0x02 and named[2.5 * s] == 0x02
    assert named[448.0] == named[465.0] == named[1e9] == named[inf] == 0x7E
    assert named[-448.0] == named[-465.0] == named[-1e9] == named[-inf] == 0xFE


def test_nan_keeps_the_nan_code():
    c = fp8_oracle.e4m3_codes(torch.tensor([float("nan"), 1.0]))
    assert c[0] & 0x7F == 0x7F and c[1] == 0x38
    assert torch.isnan(fp8_oracle.e4m3_values(c)[0])
