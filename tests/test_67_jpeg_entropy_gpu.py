"""JPEG entropy decode on the GPU: bsclip_jpeg_entropy_device against the host decoder, bit for bit -- the committed
fixtures in mixed batches at several sync_mcus, two Pillow-made pictures large enough for several workgroups per image, damaged
streams between intact neighbours, and the shard loader in GPU entropy mode against a raw shard of the same pixels."""
import io
import os

import numpy as np
import pytest
import torch

import jpeg_model as jm
import jpeg_sync_model as sm

pytestmark = pytest.mark.gpu

ROOT = jm.ROOT
TINY = os.path.join(ROOT, "tests", "golden", "tiny_shard")
FILL, TAIL = 0x5A5A, 4096


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def host():
    """{name: (bytes, host decoder's coefficients)} of the ten fixtures, decoded once."""
    return {nm: (jm.fixture_bytes(nm), coef.copy()) for nm, coef, _, _ in jm.decode_all()}


def _run(streams, sync_mcus, index_from=None):
    """One bsclip_jpeg_entropy_device launch -> (coef_dev and TAIL elements past its end as uint16, status int32 [B], batch)."""
    from bioscanclip.hip import ops
    b = sm.batch(streams, sync_mcus, index_from=index_from)
    B = len(streams)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    whole = torch.full((b["ncoef"] + TAIL,), FILL, dtype=torch.int16, device="cuda")
    status = torch.full((B,), -1, dtype=torch.int32, device="cuda")             # the library zeroes it
    rec_dev = torch.full((B, 16), -1, dtype=torch.int32, device="cuda")         # and fills these from the validated host records
    seg_dev = torch.full((B, 8), -1, dtype=torch.int32, device="cuda")
    rec_host, seg_host = torch.from_numpy(b["rec"]), torch.from_numpy(b["seg"])
    ops.jpeg_entropy_device(dev(b["bytes"]), dev(b["sync"]), dev(b["huff"]), rec_host, seg_host, rec_dev, seg_dev, B, whole, b["ncoef"], status)
    torch.cuda.synchronize()
    assert torch.equal(rec_dev.cpu(), rec_host) and torch.equal(seg_dev.cpu(), seg_host)
    return whole.cpu().numpy().view(np.uint16), status.cpu().numpy(), b


def _equal(whole, b, k, want):
    got = whole[b["coef_off"][k]:b["coef_off"][k + 1]].view(np.int16)
    return len(got) == len(want) and np.array_equal(got, want)


@pytest.mark.parametrize("sync_mcus", [1, 2, 3, 5])
def test_fixtures_equal_the_host_decoder(host, sync_mcus):
    """The ten fixtures in one batch, then the list seven times over in shuffled order: mixed sizes, samplings, tables and the
    restart file, every coefficient the host decoder's, the 4 096 elements past the end untouched, every status 0."""
    names = list(host)
    shuffled = [names[i] for i in np.random.default_rng(67).permutation(np.repeat(np.arange(len(names)), 7))]
    for order in (names, shuffled):
        whole, status, b = _run([host[nm][0] for nm in order], sync_mcus)
        assert (status == 0).all(), list(zip(order, status))
        for k, nm in enumerate(order):
            assert _equal(whole, b, k, host[nm][1]), (nm, k)
        assert (whole[b["ncoef"]:] == FILL).all() and len(whole) == b["ncoef"] + TAIL


def test_generated_pictures_equal_the_host_decoder():
    """341 x 256 4:2:0 q90 (352 MCUs, 44 segments) and 512 x 384 4:4:4 q95 (3 072 MCUs, 384 segments: six workgroups) at
    sync_mcus = 8, in one batch, so the smaller image's workgroup count differs from the grid's."""
    Image = pytest.importorskip("PIL.Image", reason="Pillow is not installed: the pictures cannot be made here")
    pytest.importorskip("PIL")
    rng = np.random.default_rng(8)
    streams = []
    for (w, h), q, sub in (((341, 256), 90, "4:2:0"), ((512, 384), 95, "4:4:4")):
        y, x = np.mgrid[0:h, 0:w]
        px = np.stack([128 + 100 * np.sin(x / 17.0 + c) * np.cos(y / 23.0 - c) for c in range(3)], axis=2) + rng.normal(0, 12, (h, w, 3))
        buf = io.BytesIO()
        Image.fromarray(np.clip(px, 0, 255).astype(np.uint8)).save(buf, format="JPEG", quality=q, subsampling=sub)
        streams.append(buf.getvalue())
    want = []
    for s in streams:
        rc, coef, _, _ = jm.entropy_decode(s)
        assert rc == 0
        want.append(coef)
    whole, status, b = _run(streams, 8)
    assert [int(n) for n in b["seg"][:, 3]] == [44, 384]
    assert (status == 0).all()
    for k in range(2):
        assert _equal(whole, b, k, want[k]), k
    assert (whole[b["ncoef"]:] == FILL).all()


def test_damaged_streams_are_flagged_and_their_neighbours_are_not(host):
    """Three damaged streams that the shared routine flags on the host under the sanitisers (tools/jpeg_segments_check.cpp; the CPU
    test pins its "flagged" lines), each between two intact images with the intact index: only its status is non-zero -- the same bits
    as on the host -- the neighbours decode to the host decoder's coefficients, and nothing is written past the end."""
    for name, at, value, want_status in sm.FLAGGED:
        good = host[name][0]
        scan = sm.parse_headers(good)["scan"]
        bad = bytearray(good)
        bad[scan + at] = value
        left, right = "c64x48_420_q90", "c20x20_grey"
        clean = [host[left][0], good, host[right][0]]
        whole, status, b = _run([clean[0], bytes(bad), clean[2]], 2, index_from=clean)
        assert status[0] == 0 and status[2] == 0 and status[1] == want_status, (name, list(status))
        assert _equal(whole, b, 0, host[left][1]) and _equal(whole, b, 2, host[right][1]), name
        assert (whole[b["ncoef"]:] == FILL).all(), name
        assert (whole[b["coef_off"][1]:b["coef_off"][2]] != FILL).any()     # the damaged image's range was still written (zero-filled)


N_SAMPLES = 11     # the ten fixtures and the first one again: batch sizes 3 and 5 both end on a ragged batch


@pytest.fixture(scope="module")
def shard_pair(tmp_path_factory):
    """A JPEG shard of the fixtures with a sync index, and a raw shard of the pixels they decode to (the NumPy model's, which
    tests/test_66_jpeg_gpu.py holds the pixel kernels to bit for bit)."""
    from bioscanclip.util import shards
    tiny = shards.Shard(TINY)
    items = (jm.decode_all() * 2)[:N_SAMPLES]
    root = tmp_path_factory.mktemp("jpeg_sync_shards")
    common = dict(barcodes=[tiny.barcode(i) for i in range(N_SAMPLES)], input_ids=np.array(tiny.input_ids[:N_SAMPLES]),
                  token_type_ids=np.array(tiny.token_type_ids[:N_SAMPLES]), attention_mask=np.array(tiny.attention_mask[:N_SAMPLES]),
                  processid=[f"JPG{i:03d}" for i in range(N_SAMPLES)],
                  taxonomy={t: [v.decode() for v in tiny.taxonomy[t][:N_SAMPLES]] for t in ("order", "family", "genus", "species")})
    shards.write_shard(str(root / "jpeg"), [jm.fixture_bytes(it[0]) for it in items], image_codec="jpeg", jpeg_sync_mcus=2, **common)
    shards.write_shard(str(root / "raw"), [jm.model_pixels(it[1], it[2], it[3]) for it in items], **common)
    return str(root / "jpeg"), str(root / "raw")


@pytest.mark.parametrize("for_training", [False, True])
@pytest.mark.parametrize("batch_size", [3, 5])
def test_loader_in_gpu_entropy_mode_equals_the_raw_shard(shard_pair, for_training, batch_size):
    """Same seeds, same 7-tuples, image tensors bit for bit, over two epochs; batch size 3 runs four batches per epoch through the
    three staging slots, so a slot's status words are read both before a refill and at the end of the iteration."""
    from bioscanclip.util import shards
    kw = dict(batch_size=batch_size, shuffle=for_training, seed=3, for_training=for_training, with_text=True)
    lj = shards.ShardLoader(shard_pair[0], entropy="gpu", **kw)
    lr = shards.ShardLoader(shard_pair[1], **kw)
    assert lj.entropy == "gpu" and lj.shard.jpeg_sync_mcus == 2 and lr.shard.image_codec == "raw" and lj._pool is None
    for epoch in (0, 1):
        lj.set_epoch(epoch)
        lr.set_epoch(epoch)
        nb = 0
        for a, b in zip(lj, lr):
            torch.cuda.synchronize()
            assert lj.last_indices == lr.last_indices and lj.last_params == lr.last_params
            assert a[0] == b[0]
            assert a[1].shape == (len(a[0]), 3, 224, 224) and torch.equal(a[1], b[1]), (epoch, nb)
            for k in (2, 3, 4, 5):
                assert torch.equal(a[k], b[k]), k
            assert torch.equal(a[6], b[6]) if for_training else a[6] == b[6]
            nb += 1
        assert nb == len(lj) == len(lr) == -(-N_SAMPLES // batch_size)
        assert not any("status_idx" in s for s in lj._slots)          # every batch's status words were looked at


def test_loader_reports_a_shard_damaged_after_it_was_written(shard_pair, tmp_path):
    """One scan byte of one sample overwritten in a copy of the shard: the iteration raises RuntimeError naming the shard and the sample."""
    import shutil
    from bioscanclip.util import shards
    path = str(tmp_path / "damaged")
    shutil.copytree(shard_pair[0], path)
    sh = shards.Shard(path)
    name, at, value, _ = sm.FLAGGED[0]
    k = jm.fixture_names().index(name)
    assert sh.image_bytes(k) == jm.fixture_bytes(name)
    off = int(sh.image_index[k][0]) + sm.parse_headers(sh.image_bytes(k))["scan"] + at
    del sh
    with open(os.path.join(path, "images.bin"), "r+b") as f:
        f.seek(off)
        f.write(bytes([value]))
    loader = shards.ShardLoader(path, 3, entropy="gpu", for_training=False)
    with pytest.raises(RuntimeError, match=rf"damaged.*samples \[{k}\]") as ei:
        for _ in loader:
            pass
    assert path in str(ei.value)


@pytest.mark.timeout(900)
def test_train_cl_decodes_a_jpeg_shard_on_the_gpu(tmp_path, capsys):
    """``train_cl.py dataset=<indexed JPEG shard> hip_jpeg_entropy=gpu``: one epoch (24 samples, batch 8), I+D+T, the default launch
    path, with the loader in GPU entropy mode."""
    import sys
    from bioscanclip.util import shards
    tiny = shards.Shard(TINY)
    names = jm.fixture_names()
    streams = [jm.fixture_bytes(names[i % len(names)]) for i in range(24)]
    path = str(tmp_path / "jpeg24")
    shards.write_shard(path, streams, [tiny.barcode(i) for i in range(24)], np.array(tiny.input_ids), np.array(tiny.token_type_ids),
                       np.array(tiny.attention_mask), [f"J{i:03d}" for i in range(24)], image_codec="jpeg",
                       jpeg_sync_mcus=shards.DEFAULT_JPEG_SYNC_MCUS)
    sys.path.insert(0, os.path.join(ROOT, "bioscan-clip_amd", "scripts"))
    import train_cl
    made = []
    init = shards.ShardLoader.__init__

    def spy(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self.entropy)
    shards.ShardLoader.__init__ = spy
    try:
        torch.manual_seed(5)
        losses = train_cl.main(["model_config=lora_vit_lora_barcode_bert_lora_bert_ssl", "model_config.batch_size=8", "model_config.epochs=1",
                                f"dataset={path}", "hip_jpeg_entropy=gpu", "debug_flag=true", f"project_root_path={tmp_path}"])
    finally:
        shards.ShardLoader.__init__ = init
    capsys.readouterr()
    assert made == ["gpu"]
    assert len(losses) == 1 and all(l == l and 0 < l < 20 for l in losses)
