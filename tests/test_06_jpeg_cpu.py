"""JPEG shards, the parts that need no GPU: the host entropy decoder through its C entry points, the NumPy model of the
pixel arithmetic against Pillow's decode of the committed fixtures, the shard container, refusals, damaged streams, and the
stand-alone sanitiser program.  tests/golden/jpeg/ is written by tools/make_jpeg_fixtures.py."""
import ctypes
import io
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_model as jm

ROOT = jm.ROOT
TINY = os.path.join(ROOT, "tests", "golden", "tiny_shard")


def test_fixture_set_is_the_one_the_decoder_has_to_face():
    m = jm.manifest()
    got = {(e["width"], e["height"], e["mode"], e["options"].get("subsampling")) for e in m["fixtures"]}
    for want in [(8, 8, "RGB", "4:4:4"), (17, 9, "RGB", "4:4:4"), (37, 29, "RGB", "4:2:0"), (33, 16, "RGB", "4:2:2"),
                 (48, 40, "RGB", "4:2:0"), (20, 20, "L", None), (31, 31, "RGB", "4:2:0"), (24, 24, "RGB", "4:4:4"), (64, 48, "RGB", "4:2:0")]:
        assert want in got, want
    by = {e["name"]: e for e in m["fixtures"]}
    assert by["c17x9_444_opt"]["options"]["optimize"] and by["c48x40_420_rst"]["options"]["restart_marker_rows"] == 1
    assert by["c31x31_420_q10"]["min"] == 0 and by["c31x31_420_q10"]["max"] == 255          # the clamp is driven to both ends
    assert all(os.path.getsize(os.path.join(jm.GOLDEN, f)) < 16384 for f in os.listdir(jm.GOLDEN))
    assert [e["name"] for e in m["refused"]] == ["p16x16_progressive"]


def test_probe_reports_the_frame():
    from bioscanclip.hip import ops
    want = {"c8x8_444": (1, 1, 3, 0), "c37x29_420_q75": (2, 2, 3, 0), "c33x16_422_q50": (2, 1, 3, 0), "c28x44_440_patched": (1, 2, 3, 0),
            "c20x20_grey": (1, 1, 1, 0), "c48x40_420_rst": (2, 2, 3, 3)}
    for e in jm.manifest()["fixtures"]:
        info = ops.jpeg_probe(jm.fixture_bytes(e["name"]))
        assert (info.width, info.height) == (e["width"], e["height"])
        assert info.pixel_bytes == 3 * e["width"] * e["height"]
        mx, my = -(-info.width // (8 * info.h_samp)), -(-info.height // (8 * info.v_samp))
        assert info.coef_count == 64 * mx * my * (info.h_samp * info.v_samp + (2 if info.components == 3 else 0))
        if e["name"] in want:
            assert (info.h_samp, info.v_samp, info.components, info.restart_interval) == want[e["name"]], e["name"]


@pytest.mark.parametrize("name", jm.fixture_names())
def test_model_is_within_the_ceiling_of_pillow(name):
    """Host entropy decode -> NumPy model of the kernel's integer arithmetic, against Pillow's pixels.  The gate is the derived
    ceiling of 5 LSB; the figure measured with libjpeg's own rounding biases is 0 on every fixture (printed, and in DESIGN 4c)."""
    rc, coef, qtab, rec = jm.entropy_decode(jm.fixture_bytes(name), guard=128)
    assert rc == 0
    got, want = jm.model_pixels(coef, qtab, rec), jm.fixture_pixels(name)
    assert got.shape == want.shape and got.dtype == np.uint8
    d = np.abs(got.astype(np.int64) - want.astype(np.int64))
    print(f"{name}: model vs Pillow max {d.max()} mean {d.mean():.4f}")
    assert d.max() <= jm.PIL_CEILING


def test_fixtures_are_fresh():
    """The committed .npy are what Pillow decodes from the committed .jpg today."""
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: the committed pixels cannot be re-derived here")
    for name in jm.fixture_names():
        fresh = np.asarray(Image.open(io.BytesIO(jm.fixture_bytes(name))).convert("RGB"), dtype=np.uint8)
        assert np.array_equal(fresh, jm.fixture_pixels(name)), name


def _write(path, codec, images, n=None):
    from bioscanclip.util import shards
    tiny = shards.Shard(TINY)
    n = len(images) if n is None else n
    shards.write_shard(path, images, [tiny.barcode(i) for i in range(n)], np.array(tiny.input_ids[:n]), np.array(tiny.token_type_ids[:n]),
                       np.array(tiny.attention_mask[:n]), [f"J{i:03d}" for i in range(n)], image_codec=codec)
    return shards.Shard(path)


def test_container_round_trip(tmp_path):
    from bioscanclip.util import shards
    names = jm.fixture_names()
    streams = [jm.fixture_bytes(nm) for nm in names]
    sh = _write(str(tmp_path / "j"), "jpeg", streams)
    assert sh.image_codec == "jpeg" and sh.meta["image_codec"] == "jpeg" and sh.meta["version"] == 1 and len(sh) == len(names)
    off = 0
    for i, (nm, s) in enumerate(zip(names, streams)):
        h, w, _ = jm.fixture_pixels(nm).shape
        assert tuple(int(v) for v in sh.image_index[i]) == (off, h, w)
        assert int(sh.image_nbytes[i]) == len(s) and sh.image_bytes(i) == s
        off += len(s)
    assert os.path.getsize(tmp_path / "j" / "images.bin") == off
    with pytest.raises(RuntimeError, match="ShardLoader"):
        sh.image(0)
    # raw shards are what they were: no codec in meta.json, no image_bytes.npy, pixels through image()
    px = [jm.fixture_pixels(nm) for nm in names]
    raw = _write(str(tmp_path / "r"), "raw", px)
    assert "image_codec" not in raw.meta and raw.image_codec == "raw" and not os.path.exists(tmp_path / "r" / "image_bytes.npy")
    assert np.array_equal(raw.image(2), px[2])
    with pytest.raises(RuntimeError, match="raw shard"):
        raw.image_bytes(0)
    tiny = shards.Shard(TINY)
    assert "image_codec" not in tiny.meta and tiny.image_codec == "raw"
    with pytest.raises(ValueError, match="image_codec"):
        _write(str(tmp_path / "x"), "png", px)
    with pytest.raises(ValueError, match="decode_threads"):
        shards.ShardLoader(sh, 2, decode_threads=17)       # refused before anything touches a device


def test_refusals_name_the_reason(tmp_path):
    from bioscanclip.hip import lib, ops
    prog = open(os.path.join(jm.GOLDEN, "p16x16_progressive.jpg"), "rb").read()
    with pytest.raises(ops.JpegRefused, match="progressive") as ei:
        ops.jpeg_probe(prog)
    assert ei.value.code == -12
    rc, _, _, _ = jm.entropy_decode(prog, guard=64)
    assert rc == -12 and "progressive" in lib.last_error()
    with pytest.raises(ValueError, match=r"image 1: .*progressive"):
        _write(str(tmp_path / "p"), "jpeg", [jm.fixture_bytes("c8x8_444"), prog])
    with pytest.raises(ValueError, match="bytes"):
        _write(str(tmp_path / "q"), "jpeg", [jm.fixture_pixels("c8x8_444")])

    # the other refusals, made by editing the headers of a good stream: each has a code of its own and decodes nothing
    good = bytearray(jm.fixture_bytes("c37x29_420_q75"))
    sof = good.index(b"\xff\xc0")

    def edited(pos, value):
        b = bytearray(good)
        b[pos] = value
        return bytes(b)
    cases = [(edited(sof + 1, 0xC1), -12, "SOF1"), (edited(sof + 1, 0xC9), -12, "arithmetic"), (edited(sof + 4, 12), -12, "12-bit"),
             (edited(sof + 11, 0x41), -14, "sampling"), (edited(sof + 14, 0x21), -14, "sampling"),
             (edited(sof + 5, 0x20), -17, "4096"), (edited(good.index(b"\xff\xdb") + 1, 0xE5), -16, "quantisation table"),
             (edited(good.index(b"\xff\xc4") + 1, 0xE5), -16, "Huffman table")]
    cmyk = bytearray(good)          # a four-component frame header (lengths kept consistent)
    cmyk[sof + 9] = 4
    cmyk[sof + 3] = 8 + 3 * 4
    cmyk[sof + 19:sof + 19] = bytes([4, 0x11, 0])
    cases.append((bytes(cmyk), -13, "4 components"))
    sos = good.index(b"\xff\xda")   # a first scan that carries one of the three components
    one = bytes(good[:sos]) + bytes([0xFF, 0xDA, 0, 8, 1, 1, 0x00, 0, 63, 0]) + bytes(good[sos + 14:])
    cases.append((one, -15, "multi-scan"))
    for data, code, word in cases:
        with pytest.raises(ops.JpegRefused, match=word) as ei:
            ops.jpeg_probe(data)
        assert ei.value.code == code, (word, ei.value.code)
        rc, coef, _, _ = jm.entropy_decode(data, guard=64, fill=0x5A5A)
        assert rc == code and (coef.view(np.uint16) == 0x5A5A).all(), word       # refused means nothing was written


@pytest.mark.parametrize("name", ["c48x40_420_rst", "c17x9_444_opt"])
def test_damaged_streams_return_a_code(name):
    """Truncation at every 7th length and single-byte damage (0x00 / 0xFF / complement) at every 5th position, through the ctypes
    entry point: each call returns 0 or a documented error code -- never a partial decode flagged as good, since the policy is
    error-not-zero-fill -- and the guard bands around coef_out stay as they were (asserted inside entropy_decode)."""
    from bioscanclip.hip import lib
    data = jm.fixture_bytes(name)
    _, clean, _, _ = jm.entropy_decode(data)
    known = {0, -1} | set(range(-18, -9))
    seen = set()
    for n in range(0, len(data), 7):
        rc, coef, _, _ = jm.entropy_decode(data[:n], guard=96)
        assert rc in known, (n, rc)
        if rc == 0:      # only the end-of-image marker (and padding bits) may go missing without harm
            assert n >= len(data) - 4 and np.array_equal(coef, clean), n
        else:
            assert lib.last_error()
        seen.add(rc)
    for i in range(0, len(data), 5):
        for v in (0x00, 0xFF, data[i] ^ 0xFF):
            if v == data[i]:
                continue
            rc, coef, _, rec = jm.entropy_decode(data[:i] + bytes([v]) + data[i + 1:], guard=96)
            assert rc in known, (i, v, rc)
            seen.add(rc)
            if rc == 0:
                assert 64 * int(rec[12]) == len(coef)
    assert -10 in seen and -11 in seen and 0 in seen
    rc, again, _, _ = jm.entropy_decode(data)
    assert rc == 0 and np.array_equal(again, clean)


def test_entropy_decode_is_thread_safe():
    """Eight threads decode different fixtures at once, many times over; every result equals the single-threaded one and a failing
    call's message stays with the thread that made it."""
    from concurrent.futures import ThreadPoolExecutor
    from bioscanclip.hip import lib
    names = jm.fixture_names()
    ref = {nm: jm.entropy_decode(jm.fixture_bytes(nm))[1].copy() for nm in names}
    prog = open(os.path.join(jm.GOLDEN, "p16x16_progressive.jpg"), "rb").read()

    def work(t):
        for r in range(25):
            nm = names[(t + r) % len(names)]
            if (t + r) % 4 == 0:
                rc, _, _, _ = jm.entropy_decode(prog)
                assert rc == -12 and "progressive" in lib.last_error()
            rc, coef, _, _ = jm.entropy_decode(jm.fixture_bytes(nm))
            assert rc == 0 and np.array_equal(coef, ref[nm]), nm
        return True
    with ThreadPoolExecutor(max_workers=8) as pool:
        assert all(pool.map(work, range(8)))


def test_pixels_entry_point_validates_on_the_host():
    """bsclip_jpeg_pixels checks its records and capacities before anything is launched, so bad calls fail cleanly without a GPU."""
    from bioscanclip.hip import lib
    h = lib.load()
    _, coef, qtab, rec = jm.entropy_decode(jm.fixture_bytes("c37x29_420_q75"))
    one = ctypes.c_void_p(4096)     # non-null, aligned: every check below comes before any dereference of a device pointer

    def call(**kw):
        a = dict(coef=one, n=len(coef), qtab=one, slots=3, rec=rec, recd=one, B=1, scratch=one, sb=len(coef), out=one, cap=3 * 37 * 29)
        a.update(kw)
        r = np.ascontiguousarray(a["rec"], dtype=np.int32)
        return h.bsclip_jpeg_pixels(a["coef"], a["n"], a["qtab"], a["slots"], ctypes.c_void_p(r.ctypes.data), a["recd"], a["B"],
                                    a["scratch"], a["sb"], a["out"], a["cap"], None)
    for k in ("coef", "qtab", "recd", "scratch", "out"):
        assert call(**{k: None}) == -1 and "null pointer" in lib.last_error(), k
    assert call(cap=3 * 37 * 29 - 1) == -1 and "out_capacity" in lib.last_error()
    assert call(sb=len(coef) - 1) == -1 and "scratch_bytes" in lib.last_error()
    assert call(n=len(coef) - 64) == -1 and "coef_count" in lib.last_error()
    assert call(slots=2) == -1 and "qtab_slots" in lib.last_error()
    assert call(B=0) == -1 and "B=0" in lib.last_error()
    for k in ("coef", "qtab", "scratch", "out"):
        assert call(**{k: ctypes.c_void_p(4096 + 8)}) == -1 and "aligned" in lib.last_error(), k
    bad = rec.copy()
    bad[4] = 49                      # a fourth MCU column: a quarter of the blocks would be missing
    assert call(rec=bad, cap=3 * 49 * 29) == -1 and "blocks" in lib.last_error()
    bad = rec.copy()
    bad[12] -= 1
    assert call(rec=bad) == -1 and "blocks" in lib.last_error()
    bad = rec.copy()
    bad[7] = 3
    assert call(rec=bad) == -1 and "not decodable" in lib.last_error()
    bad = rec.copy()
    bad[0] = 32                      # offsets are whole blocks
    assert call(rec=bad, n=len(coef) + 64, sb=len(coef) + 64) == -1 and "multiple of 64" in lib.last_error()
    bad = rec.copy()
    bad[2] = 1
    assert call(rec=bad) == -1 and "out_capacity" in lib.last_error()
    assert h.bsclip_jpeg_pixels_workspace_bytes(len(coef)) == len(coef) and h.bsclip_jpeg_pixels_workspace_bytes(0) == -1


def test_sanitised_entropy_check_program(tmp_path):
    """tools/jpeg_entropy_check.cpp under AddressSanitizer + UBSan on the host: every fixture intact, truncated at every length and
    with each of its first 600 bytes damaged three ways."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ / g++ / clang++) on PATH: the sanitiser program cannot be built here")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("LD_PRELOAD is set: a sanitised program must be the first runtime in its process, run this where nothing is preloaded")
    exe = str(tmp_path / "jpeg_entropy_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    trivial = tmp_path / "trivial.cpp"       # decided up front: can this compiler link and run anything with these flags?
    trivial.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, *flags, str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "trivial")]).returncode != 0:
        pytest.skip(f"{cxx} cannot build and run a trivial program with {' '.join(flags[3:])}: no sanitiser runtime here")
    build = subprocess.run([cxx, *flags, "-I", os.path.join(ROOT, "bioscan-clip_amd", "csrc"),
                            os.path.join(ROOT, "tools", "jpeg_entropy_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, jm.GOLDEN], capture_output=True, text=True)
    print(run.stdout.strip())
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout
