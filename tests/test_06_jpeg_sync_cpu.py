"""The JPEG sync index and the segment decoder, the parts that need no GPU: the index's properties on the committed
fixtures, a plain-Python segment decoder (tests/jpeg_sync_model.py, from the specification) against the host decoder, the
stand-alone sanitiser program, the shard container and the refusals, and the host-side validation of bsclip_jpeg_entropy_device."""
import ctypes
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import jpeg_model as jm
import jpeg_sync_model as sm

ROOT = jm.ROOT
TINY = os.path.join(ROOT, "tests", "golden", "tiny_shard")
SYNCS = (1, 2, 3, 5, 4096)


@pytest.fixture(scope="module")
def fixtures():
    """{name: (bytes, parsed headers, host decoder's coefficients)} of the ten committed fixtures, decoded once."""
    out = {}
    for name in jm.fixture_names():
        data = jm.fixture_bytes(name)
        rc, coef, _, _ = jm.entropy_decode(data)
        assert rc == 0
        out[name] = (data, sm.parse_headers(data), coef.copy())
    assert len(out) == 10
    return out


def _last_dc(hdr, coef, mcu):
    """DC coefficient of each component's last block in MCU ``mcu`` of the host decoder's raster."""
    my, mx = divmod(mcu, hdr["mcus_x"])
    out, off = [], 0
    for h, v, _, _ in hdr["comps"]:
        bw, bh = hdr["mcus_x"] * h, hdr["mcus_y"] * v
        out.append(int(coef[off + 64 * ((my * v + v - 1) * bw + mx * h + h - 1)]))
        off += 64 * bw * bh
    return out


def _unpack(entry, ncomp):
    cb, cr = int(entry[3]) & 0xFFFF, (int(entry[3]) >> 16) & 0xFFFF
    return [int(entry[2]), cb - 65536 if cb >= 32768 else cb, cr - 65536 if cr >= 32768 else cr][:ncomp]


@pytest.mark.parametrize("sync_mcus", SYNCS)
def test_index_properties(fixtures, sync_mcus):
    from bioscanclip.hip import lib, ops
    h = lib.load()
    for name, (data, hdr, coef) in fixtures.items():
        nmcu, R, nc = hdr["mcus_x"] * hdr["mcus_y"], hdr["restart"], len(hdr["comps"])
        firsts = sm.segment_firsts(nmcu, R, sync_mcus)
        src = np.frombuffer(data, dtype=np.uint8)
        assert h.bsclip_jpeg_sync_index(sm.ptr(src), src.size, sync_mcus, None, 0) == len(firsts), name   # the count, without a buffer
        idx = ops.jpeg_sync_index(data, sync_mcus)
        assert idx.shape == (len(firsts), 4) and idx.dtype == np.int32
        assert list(idx[0]) == [8 * hdr["scan"], 0, 0, 0], name
        assert list(idx[:, 1]) == firsts, name
        assert (np.diff(idx[:, 0]) > 0).all() and (np.diff(idx[:, 1]) > 0).all(), name
        for e in idx:
            byte = int(e[0]) >> 3
            assert hdr["scan"] <= byte < len(data) - 2
            assert not (data[byte] == 0x00 and data[byte - 1] == 0xFF), (name, "a stuffed byte")
            assert not (data[byte] == 0xFF and data[byte + 1] != 0x00), (name, "a marker")
            starts_interval = R and int(e[1]) % R == 0
            want = [0] * nc if int(e[1]) == 0 or starts_interval else _last_dc(hdr, coef, int(e[1]) - 1)
            assert _unpack(e, nc) == want, (name, int(e[1]))
            if nc == 1:
                assert int(e[3]) == 0
    if sync_mcus == 2:
        data, hdr, _ = fixtures["c48x40_420_rst"]
        assert hdr["restart"] == 3
        idx = ops.jpeg_sync_index(data, 2)
        assert list(idx[:, 1]) == [0, 2, 3, 5, 6, 8]
        at_restart = idx[idx[:, 1] % 3 == 0]
        assert len(at_restart) == 3 and (at_restart[:, 2:] == 0).all()     # 9 MCUs: intervals at 0, 3, 6
        for e in at_restart[1:]:          # right behind its RSTn marker, on a byte boundary
            b = int(e[0]) >> 3
            assert int(e[0]) & 7 == 0 and data[b - 2] == 0xFF and 0xD0 <= data[b - 1] <= 0xD7


def test_index_refusals():
    from bioscanclip.hip import lib, ops
    good = jm.fixture_bytes("c37x29_420_q75")
    for bad in (0, -3):
        with pytest.raises(ops.JpegRefused, match="sync_mcus") as ei:
            ops.jpeg_sync_index(good, bad)
        assert ei.value.code == -1
    prog = open(os.path.join(jm.GOLDEN, "p16x16_progressive.jpg"), "rb").read()
    with pytest.raises(ops.JpegRefused, match="progressive") as ei:
        ops.jpeg_sync_index(prog, 2)
    assert ei.value.code == -12
    for n in (len(good) - 40, len(good) // 2):                 # what the decoder refuses, with the decoder's code
        rc, _, _, _ = jm.entropy_decode(good[:n])
        assert rc == -10
        with pytest.raises(ops.JpegRefused) as ei:
            ops.jpeg_sync_index(good[:n], 2)
        assert ei.value.code == rc
    h = lib.load()
    src = np.frombuffer(good, dtype=np.uint8)
    out = np.full((2, 4), -7, dtype=np.int32)                    # 6 MCUs at sync_mcus = 2 need three entries
    assert h.bsclip_jpeg_sync_index(sm.ptr(src), src.size, 2, sm.ptr(out), 2) == -1 and "entries" in lib.last_error()
    assert (out == -7).all()
    # 2^28 bytes and more: refused from the length alone, before a byte is read
    assert h.bsclip_jpeg_sync_index(sm.ptr(src), 1 << 28, 2, None, 0) == -1 and "2^28" in lib.last_error()


@pytest.mark.parametrize("sync_mcus", [1, 3])
def test_python_model_decodes_every_segment_from_its_entry_alone(fixtures, sync_mcus):
    from bioscanclip.hip import ops
    near_stuffing = 0
    for name, (data, hdr, coef) in fixtures.items():
        want = sm.raster(hdr, coef)
        nmcu = hdr["mcus_x"] * hdr["mcus_y"]
        idx = ops.jpeg_sync_index(data, sync_mcus)
        got = {}
        for j in reversed(range(len(idx))):
            count = (int(idx[j + 1][1]) if j + 1 < len(idx) else nmcu) - int(idx[j][1])
            blocks, end, pred = sm.decode_segment(data, hdr, idx[j], count)
            assert not set(blocks) & set(got)
            got.update(blocks)
            same_interval = j + 1 < len(idx) and not (hdr["restart"] and int(idx[j + 1][1]) % hdr["restart"] == 0)
            if same_interval:
                assert end == int(idx[j + 1][0]) and pred[:len(hdr["comps"])] == _unpack(idx[j + 1], len(hdr["comps"])), (name, j)
            byte = int(idx[j][0]) >> 3
            near_stuffing += any(data[q - 2:q] == b"\xff\x00" for q in (byte, byte - 1) if q - 2 >= hdr["scan"])
        assert got == want, name
    print(f"sync_mcus={sync_mcus}: {near_stuffing} segments start within two bytes after a stuffed pair")
    if sync_mcus == 1:
        data, hdr, _ = fixtures["c24x24_444_q100"]
        assert data[hdr["scan"]:].count(b"\xff\x00") == 7
        assert near_stuffing >= 1


def test_sanitised_segments_check_program(tmp_path):
    """tools/jpeg_segments_check.cpp under AddressSanitizer + UBSan on the host: the shared segment routine on every fixture at
    sync_mcus 1, 2, 3, 5, segments in reverse order into a guarded buffer, then against damaged and cut streams with the intact index."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ / g++ / clang++) on PATH: the sanitiser program cannot be built here")
    if os.environ.get("LD_PRELOAD"):
        pytest.skip("LD_PRELOAD is set: a sanitised program must be the first runtime in its process, run this where nothing is preloaded")
    exe = str(tmp_path / "jpeg_segments_check")
    flags = ["-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    trivial = tmp_path / "trivial.cpp"       # decided up front: can this compiler link and run anything with these flags?
    trivial.write_text("int main() { return 0; }\n")
    probe = subprocess.run([cxx, *flags, str(trivial), "-o", str(tmp_path / "trivial")], capture_output=True, text=True)
    if probe.returncode != 0 or subprocess.run([str(tmp_path / "trivial")]).returncode != 0:
        pytest.skip(f"{cxx} cannot build and run a trivial program with {' '.join(flags[3:])}: no sanitiser runtime here")
    build = subprocess.run([cxx, *flags, "-I", os.path.join(ROOT, "bioscan-clip_amd", "csrc"),
                            os.path.join(ROOT, "tools", "jpeg_segments_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([exe, jm.GOLDEN], capture_output=True, text=True)
    print(run.stdout.strip().splitlines()[-1])
    assert run.returncode == 0, run.stdout + run.stderr
    assert " 0 failures" in run.stdout
    assert "gave status 0 with different coefficients" in run.stdout        # reported, not gated: a damaged byte can be a valid code
    for name, at, value, status in sm.FLAGGED:                               # the three streams the GPU test replays
        assert f"flagged {name} sync=2 scan+{at} value=0x{value:02X} status={status}\n" in run.stdout


def _write(path, streams, **kw):
    from bioscanclip.util import shards
    tiny = shards.Shard(TINY)
    n = len(streams)
    shards.write_shard(path, streams, [tiny.barcode(i) for i in range(n)], np.array(tiny.input_ids[:n]), np.array(tiny.token_type_ids[:n]),
                       np.array(tiny.attention_mask[:n]), [f"J{i:03d}" for i in range(n)], **kw)
    return shards.Shard(path)


def test_container_and_refusals(tmp_path, monkeypatch):
    import torch
    from bioscanclip.hip import ops
    from bioscanclip.util import shards
    names = jm.fixture_names()
    streams = [jm.fixture_bytes(nm) for nm in names]
    plain = _write(str(tmp_path / "plain"), streams, image_codec="jpeg")
    assert "jpeg_sync_mcus" not in plain.meta
    assert not [f for f in os.listdir(tmp_path / "plain") if f.startswith("image_sync")]
    assert set(plain.meta) == {"format", "version", "n", "split", "dataset", "text_len", "image_codec"} and plain.meta["version"] == 1
    assert plain.image_sync is None and plain.jpeg_sync_mcus is None

    with2 = _write(str(tmp_path / "with2"), streams, image_codec="jpeg", jpeg_sync_mcus=2)
    per = [ops.jpeg_sync_index(s, 2) for s in streams]
    sync, offs = np.load(tmp_path / "with2" / "image_sync.npy"), np.load(tmp_path / "with2" / "image_sync_offsets.npy")
    assert sync.dtype == np.int32 and sync.shape == (sum(len(p) for p in per), 4)
    assert offs.dtype == np.int64 and offs.shape == (len(names) + 1,) and list(offs) == list(np.concatenate([[0], np.cumsum([len(p) for p in per])]))
    assert np.array_equal(sync, np.concatenate(per)) and with2.meta["jpeg_sync_mcus"] == 2 and with2.meta["version"] == 1
    assert with2.jpeg_sync_mcus == 2 and np.array_equal(with2.image_sync, sync)
    for f in os.listdir(tmp_path / "plain"):        # file for file the same otherwise
        if f != "meta.json":
            assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "with2" / f, "rb").read(), f

    shards.add_jpeg_sync_index(str(tmp_path / "plain"), sync_mcus=2)
    listing = sorted(os.listdir(tmp_path / "plain"))
    assert listing == sorted(os.listdir(tmp_path / "with2"))
    for f in listing:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "with2" / f, "rb").read(), f
    before = {f: open(tmp_path / "plain" / f, "rb").read() for f in listing}
    shards.add_jpeg_sync_index(str(tmp_path / "plain"), sync_mcus=2)
    assert {f: open(tmp_path / "plain" / f, "rb").read() for f in sorted(os.listdir(tmp_path / "plain"))} == before
    assert shards.Shard(str(tmp_path / "plain")).jpeg_sync_mcus == 2
    shards.add_jpeg_sync_index(str(tmp_path / "plain"), sync_mcus=3)            # another spacing replaces the index
    again = shards.Shard(str(tmp_path / "plain"))
    assert again.jpeg_sync_mcus == 3 and np.array_equal(again.image_sync, np.concatenate([ops.jpeg_sync_index(s, 3) for s in streams]))
    assert sorted(os.listdir(tmp_path / "plain")) == listing                     # no temporary file left behind

    for bad in (0, -1, 2.5, True):
        with pytest.raises(ValueError, match="jpeg_sync_mcus"):
            _write(str(tmp_path / "bad"), streams, image_codec="jpeg", jpeg_sync_mcus=bad)
    with pytest.raises(ValueError, match="jpeg_sync_mcus"):
        _write(str(tmp_path / "bad"), [jm.fixture_pixels(nm) for nm in names], image_codec="raw", jpeg_sync_mcus=2)
    with pytest.raises(ValueError, match="JPEG shard"):
        shards.add_jpeg_sync_index(TINY)

    # the loader's refusals come before a device is touched: any torch.cuda call fails this test
    def touched(*a, **k):
        raise AssertionError("a device call before the refusal")
    for fn in ("Stream", "current_device", "set_device", "Event"):
        monkeypatch.setattr(torch.cuda, fn, touched)
    unindexed = _write(str(tmp_path / "unindexed"), streams[:3], image_codec="jpeg")
    with pytest.raises(ValueError, match="add_jpeg_sync_index"):
        shards.ShardLoader(TINY, 2, entropy="gpu")                     # a raw shard
    with pytest.raises(ValueError, match="add_jpeg_sync_index"):
        shards.ShardLoader(unindexed, 2, entropy="gpu")                # a JPEG shard without an index
    for src in (with2, TINY):
        with pytest.raises(ValueError, match="entropy must be one of"):
            shards.ShardLoader(src, 2, entropy="device")
    sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
    import train_cl
    with pytest.raises(ValueError, match="hip_jpeg_entropy"):
        train_cl.main(["model_config=lora_vit_lora_barcode_bert_lora_bert_ssl", f"dataset={tmp_path / 'with2'}", "hip_jpeg_entropy=cpu",
                       "debug_flag=true", f"project_root_path={tmp_path}"])


def test_entropy_device_entry_point_validates_on_the_host(fixtures):
    """bsclip_jpeg_entropy_device checks its records, segment records and capacities before anything is launched or copied, so bad
    calls fail cleanly without a GPU."""
    from bioscanclip.hip import lib
    h = lib.load()
    b = sm.batch([fixtures["c37x29_420_q75"][0], fixtures["c48x40_420_rst"][0]], 2, gap=0)
    one = ctypes.c_void_p(4096)     # non-null, aligned: every check below comes before any dereference of a device pointer

    def call(**kw):
        a = dict(bytes=one, cap=len(b["bytes"]), sync=one, ents=len(b["sync"]), huff=one, slots=2, rec=b["rec"], seg=b["seg"], recd=one,
                 segd=one, B=2, coef=one, n=b["ncoef"], status=one)
        a.update(kw)
        r, s = np.ascontiguousarray(a["rec"], dtype=np.int32), np.ascontiguousarray(a["seg"], dtype=np.int32)
        return h.bsclip_jpeg_entropy_device(a["bytes"], a["cap"], a["sync"], a["ents"], a["huff"], a["slots"], sm.ptr(r), sm.ptr(s), a["recd"],
                                            a["segd"], a["B"], a["coef"], a["n"], a["status"], None)

    def edited(which, row, col, value):
        m = b[which].copy()
        m[row, col] = value
        return {which: m}
    for k in ("bytes", "sync", "huff", "recd", "segd", "coef", "status"):
        assert call(**{k: None}) == -1 and "null pointer" in lib.last_error(), k
    for k in ("sync", "coef"):
        assert call(**{k: ctypes.c_void_p(4096 + 8)}) == -1 and "aligned" in lib.last_error(), k
    assert call(B=0) == -1 and "B=0" in lib.last_error()
    assert call(cap=1 << 31) == -1 and "bytes_capacity" in lib.last_error()
    assert call(cap=len(b["bytes"]) - 1) == -1 and "bytes_capacity" in lib.last_error()              # byte range
    assert call(**edited("seg", 0, 0, -1)) == -1 and "bytes_capacity" in lib.last_error()
    assert call(**edited("seg", 0, 1, 1 << 28), cap=(1 << 31) - 1) == -1 and "2^28" in lib.last_error()
    assert call(ents=len(b["sync"]) - 1) == -1 and "sync_entries" in lib.last_error()                # index range
    assert call(**edited("seg", 1, 2, -1)) == -1 and "sync_entries" in lib.last_error()
    assert call(**edited("seg", 0, 3, int(b["seg"][0, 3]) - 1)) == -1 and "imply" in lib.last_error()  # entry count against the frame
    assert call(**edited("seg", 1, 4, 3)) == -1 and "imply" in lib.last_error()
    assert call(**edited("seg", 1, 4, 0)) == -1 and "sync_mcus" in lib.last_error()
    assert call(**edited("rec", 1, 13, 4)) == -1 and "imply" in lib.last_error()                      # another restart interval
    assert call(slots=1) == -1 and "huff_slots" in lib.last_error()
    assert call(n=b["ncoef"] - 64) == -1 and "coef_count" in lib.last_error()                         # coefficient range
    assert call(**edited("rec", 0, 0, 32)) == -1 and "multiple of 64" in lib.last_error()
    assert call(**edited("rec", 0, 12, int(b["rec"][0, 12]) + 1)) == -1 and "blocks" in lib.last_error()
    assert call(**edited("rec", 0, 7, 3)) == -1 and "not decodable" in lib.last_error()
    assert call(**edited("rec", 0, 14, 0x100)) == -1 and "selector" in lib.last_error()
