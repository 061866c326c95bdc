"""Pre-decoded shards: the data side of the input pipeline (reference bioscanclip/util/dataset.py:97-275).

The reference keeps a split as datasets of one HDF5 file (DATA.md:23-35) and decodes a JPEG per ``__getitem__`` on a DataLoader
worker.  h5py and a JPEG decoder are absent from this image, and at >= 6 k images/s per GPU a CPU decode per sample is what
starves the step, so the stored form here is what the GPU pipeline consumes directly -- one directory per split:

    meta.json                       {"format": "bsclip-shard", "version": 1, "n", "split", "dataset", "text_len"}
                                    (+ "image_codec": "jpeg" in a JPEG shard; absent = raw)
    images.bin                      decoded uint8 H x W x 3 pixels of every sample, back to back
                                    (JPEG shard: the samples' JPEG streams, back to back)
    image_index.npy                 int64 [n, 3]: byte offset into images.bin, H, W
    image_bytes.npy                 int64 [n]: length of each stream (JPEG shards only)
    image_coefs.npy                 int64 [n]: quantised coefficients each stream decodes to (JPEG shards only; lays a batch out
                                    without parsing the streams first)
    image_sync.npy                  int32 [entries, 4]: the streams' sync-index entries, back to back (optional: JPEG shards written
                                    with ``jpeg_sync_mcus`` or indexed later by ``add_jpeg_sync_index``; meta "jpeg_sync_mcus")
    image_sync_offsets.npy          int64 [n + 1]: first entry of each stream in image_sync.npy (with it)
    barcodes.bin                    the nucleotide strings (ASCII), back to back      (HDF5 "barcode")
    barcode_offsets.npy             int64 [n + 1]
    language_tokens_input_ids.npy   int64 [n, text_len]                               (HDF5 datasets of the same names)
    language_tokens_token_type_ids.npy, language_tokens_attention_mask.npy
    processid.npy                   bytes [n]   (HDF5 "processid" for BIOSCAN-5M, "image_file" for BIOSCAN-1M: dataset.py:243-246)
    labels.npy                      int64 [n]   training labels (dataset.py:135-142: the sample index unless a label array is given)
    order.npy, family.npy, genus.npy, species.npy   bytes [n]  (get_array_of_label_dicts, dataset.py:51-62: evaluation labels)

Every array is memory-mapped; nothing is loaded whole.  ``convert_hdf5_split`` writes this layout from the reference's HDF5 file
wherever h5py exists (not in this image: documented, exercised by nothing here).

A JPEG shard (``image_codec="jpeg"``) keeps the dataset's own bytes -- several times smaller than decoded pixels -- and
the loader decodes them without a CPU pixel path: loader threads Huffman-decode each stream into quantised coefficients
(``bsclip_jpeg_entropy_decode``, host only, the GIL released), the device does the arithmetic (``bsclip_jpeg_pixels``) straight
into the uint8 staging buffer the augmentation kernels read.  Only streams the decoder takes are ever written: baseline, 8-bit,
grey or YCbCr 4:4:4 / 4:2:2 / 4:4:0 / 4:2:0, one scan.

``ShardLoader(..., entropy="gpu")`` moves the Huffman decoding to the device as well (``bsclip_jpeg_entropy_device``): the loader only
copies the stored bytes, their sync-index entries and the tables parsed from their headers, about a twelfth of the coefficients'
bytes.  It needs the shard's sync index, which records every ``jpeg_sync_mcus`` MCUs where a code starts and what the DC predictors
are, so that the segments between entries decode side by side, one lane each.  The default stays ``"host"``.

``ShardLoader`` yields the reference's 7-tuple ``(processid, image, dna, input_ids, token_type_ids, attention_mask, label)``
(dataset.py:267-275) with ``image`` f32 [B, 3, 224, 224] and ``dna`` int64 [B, 133] already on the device:
  * sample order: ``prepare()`` (dataset.py:41-48) = ``DistributedSampler(num_replicas, rank, shuffle, drop_last=True)`` -- the
    same torch class, so ``set_epoch`` reshuffles exactly as the reference's loader does -- batched without dropping the tail;
  * a producer thread gathers batch k+1 from the memory-mapped arrays into PINNED staging buffers while batch k trains, then, on
    a side HIP stream, copies it to the device and runs the two per-sample transforms there (``GpuAugment``: Resize 256 ->
    RandomResizedCrop 224 -> flips -> rotation, or Resize -> CenterCrop for evaluation; ``tokenize_barcodes``); the consumer's
    stream waits on the batch's event, the host never blocks on the copy.  Three staging slots; a slot's pinned buffers are refilled
    only after its previous copies have executed; the tensors handed to the consumer are fresh allocations of the side stream
    (``record_stream`` keeps the allocator from recycling them under the consumer).
"""
import json
import os
import queue
import threading
import time

import numpy as np
import torch

FORMAT, VERSION = "bsclip-shard", 1
CODECS = ("raw", "jpeg")
MAX_DECODE_THREADS = 16
ENTROPY_MODES = ("host", "gpu")
LABEL_MODES = (None, "ids")
DEFAULT_JPEG_SYNC_MCUS = 4     # the sweep over {2, 4, 8, 16, 32} on the bench pictures
_TAXA = ("order", "family", "genus", "species")
_TEXT = ("language_tokens_input_ids", "language_tokens_token_type_ids", "language_tokens_attention_mask")


def write_shard(path, images, barcodes, input_ids, token_type_ids, attention_mask, processid, labels=None, taxonomy=None,
                split="train", dataset="bioscan_1m", image_codec="raw", jpeg_sync_mcus=None):
    """images: sequence of uint8 [H, W, 3] arrays (sizes may differ); barcodes: sequence of str; the three text arrays
    int [n, text_len]; processid: sequence of str; labels: int [n] (default: the sample index, dataset.py:139);
    taxonomy: dict order/family/genus/species -> sequence of str (default: empty strings).
    ``image_codec="jpeg"``: images is a sequence of ``bytes``, each a JPEG stream, stored as it is.  Every stream is probed AND
    entropy-decoded here (host only), so a shard never holds one the loader's decoder refuses or finds damaged: every stream is
    looked at, then ValueError names the first ten offenders and their reasons.
    ``jpeg_sync_mcus`` (an int >= 1, JPEG shards only): also write the sync index that ``ShardLoader(entropy="gpu")`` needs, one entry
    every that many MCUs (``DEFAULT_JPEG_SYNC_MCUS`` is the measured choice); ``None`` writes exactly the files a shard had before."""
    if image_codec not in CODECS:
        raise ValueError(f"image_codec must be one of {CODECS}, got {image_codec!r}")
    if jpeg_sync_mcus is not None:
        if image_codec != "jpeg":
            raise ValueError("jpeg_sync_mcus belongs to image_codec='jpeg'")
        jpeg_sync_mcus = _check_sync_mcus(jpeg_sync_mcus)
    sync = []
    os.makedirs(path, exist_ok=True)
    n = len(barcodes)
    assert len(processid) == n and len(input_ids) == n
    index = np.zeros((n, 3), dtype=np.int64)
    nbytes, ncoefs, refused = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), []
    off, seen = 0, 0
    with open(os.path.join(path, "images.bin"), "wb") as f:
        for i, im in enumerate(images):                       # any iterable: images are streamed to disk one at a time
            if image_codec == "jpeg":
                seen += 1
                try:
                    h, w, ncoefs[i] = _check_jpeg(im, i)
                except ValueError as exc:
                    refused.append(str(exc))
                    continue
                if not refused:               # after a refusal the rest is only checked, to name more than the first offender
                    index[i] = (off, h, w)
                    nbytes[i] = len(im)
                    f.write(im)
                    off += len(im)
                    if jpeg_sync_mcus is not None:
                        sync.append(_sync_index(im, i, jpeg_sync_mcus))
                continue
            im = np.ascontiguousarray(np.asarray(im, dtype=np.uint8))
            assert im.ndim == 3 and im.shape[2] == 3, "images must be decoded uint8 H x W x 3"
            index[i] = (off, im.shape[0], im.shape[1])
            f.write(im.tobytes())
            off += im.size
            seen += 1
    if refused:
        raise ValueError(f"{len(refused)} of {seen} streams cannot go into a JPEG shard: " + "; ".join(refused[:10]))
    assert seen == n, f"{seen} images for {n} barcodes"
    np.save(os.path.join(path, "image_index.npy"), index)
    if image_codec == "jpeg":
        np.save(os.path.join(path, "image_bytes.npy"), nbytes)
        np.save(os.path.join(path, "image_coefs.npy"), ncoefs)
    if jpeg_sync_mcus is not None:
        _save_sync(path, sync, np.save)
    offs = np.zeros(n + 1, dtype=np.int64)
    with open(os.path.join(path, "barcodes.bin"), "wb") as f:
        for i, s in enumerate(barcodes):
            b = s.encode("ascii", "replace") if isinstance(s, str) else bytes(s)
            f.write(b)
            offs[i + 1] = offs[i] + len(b)
    np.save(os.path.join(path, "barcode_offsets.npy"), offs)
    for name, arr in zip(_TEXT, (input_ids, token_type_ids, attention_mask)):
        np.save(os.path.join(path, name + ".npy"), np.asarray(arr, dtype=np.int64).reshape(n, -1))
    np.save(os.path.join(path, "processid.npy"), np.asarray([str(p).encode() for p in processid], dtype=np.bytes_))
    np.save(os.path.join(path, "labels.npy"), np.arange(n, dtype=np.int64) if labels is None else np.asarray(labels, dtype=np.int64))
    for t in _TAXA:
        vals = [""] * n if taxonomy is None else list(taxonomy[t])
        np.save(os.path.join(path, t + ".npy"), np.asarray([str(v).encode() for v in vals], dtype=np.bytes_))
    meta = {"format": FORMAT, "version": VERSION, "n": n, "split": split, "dataset": dataset,
            "text_len": int(np.asarray(input_ids).reshape(n, -1).shape[1])}
    if image_codec != "raw":       # absent = raw: shards written before the codec existed, and raw ones since, read the same
        meta["image_codec"] = image_codec
    if jpeg_sync_mcus is not None:
        meta["jpeg_sync_mcus"] = jpeg_sync_mcus
    with open(os.path.join(path, "meta.json"), "w") as f:
        json.dump(meta, f)


def _check_jpeg(data, i):
    """(H, W, coefficient count) of one JPEG stream that the loader will be able to decode; ValueError otherwise."""
    from bioscanclip.hip import ops
    if not isinstance(data, (bytes, bytearray)):
        raise ValueError(f"image {i}: image_codec='jpeg' takes the JPEG stream as bytes, got {type(data).__name__}")
    try:
        info = ops.jpeg_probe(data)
        coef = np.empty(int(info.coef_count), dtype=np.int16)
        qtab, rec = np.empty(192, dtype=np.uint16), np.empty(16, dtype=np.int32)
        src = np.frombuffer(data, dtype=np.uint8)
        ops.jpeg_entropy_decode(src.ctypes.data, src.size, coef.ctypes.data, coef.size, qtab.ctypes.data, rec.ctypes.data)
    except ops.JpegRefused as exc:
        raise ValueError(f"image {i}: {exc} (code {exc.code}); re-encode it as baseline JPEG or write a raw shard") from exc
    return int(info.height), int(info.width), int(info.coef_count)


def _check_sync_mcus(v):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
        raise ValueError(f"jpeg_sync_mcus must be an integer >= 1, got {v!r}")
    return int(v)


def _sync_index(data, i, sync_mcus):
    from bioscanclip.hip import ops
    try:
        return ops.jpeg_sync_index(data, sync_mcus)
    except ops.JpegRefused as exc:
        raise ValueError(f"image {i}: {exc} (code {exc.code}): the stream cannot be indexed") from exc


def _save_sync(path, sync, save):
    """image_sync.npy / image_sync_offsets.npy from the per-stream entry arrays."""
    offs = np.concatenate([[0], np.cumsum([len(a) for a in sync])]).astype(np.int64)
    save(os.path.join(path, "image_sync.npy"), np.concatenate(sync).astype(np.int32).reshape(-1, 4) if sync else np.zeros((0, 4), np.int32))
    save(os.path.join(path, "image_sync_offsets.npy"), offs)


def add_jpeg_sync_index(path, sync_mcus=None):
    """Index an existing JPEG shard in place (host only): writes the same ``image_sync.npy`` / ``image_sync_offsets.npy`` and
    ``meta["jpeg_sync_mcus"]`` as ``write_shard(..., jpeg_sync_mcus=sync_mcus)`` would have.  The arrays are written under temporary
    names and renamed, and meta.json is replaced last and atomically, so a reader never sees an index its meta.json does not
    describe (a shard already indexed at another spacing first loses its meta key, the same way).  ``sync_mcus=None``:
    ``DEFAULT_JPEG_SYNC_MCUS``."""
    sync_mcus = _check_sync_mcus(DEFAULT_JPEG_SYNC_MCUS if sync_mcus is None else sync_mcus)
    sh = Shard(path)
    if sh.image_codec != "jpeg":
        raise ValueError(f"{path}: only a JPEG shard has streams to index (image_codec is {sh.image_codec!r})")
    sync = []
    for i in range(sh.n):
        o = int(sh.image_index[i][0])
        sync.append(_sync_index(sh.images[o:o + int(sh.image_nbytes[i])], i, sync_mcus))

    def save(name, arr):
        tmp = name + ".tmp.npy"
        np.save(tmp, arr)
        os.replace(tmp, name)

    def save_meta(meta):
        tmp = os.path.join(path, "meta.json.tmp")
        with open(tmp, "w") as f:
            json.dump(meta, f)
        os.replace(tmp, os.path.join(path, "meta.json"))
    if sh.jpeg_sync_mcus not in (None, sync_mcus):
        save_meta({k: v for k, v in sh.meta.items() if k != "jpeg_sync_mcus"})
    _save_sync(path, sync, save)
    save_meta(dict(sh.meta, jpeg_sync_mcus=sync_mcus))


def is_shard(path):
    return isinstance(path, str) and os.path.isfile(os.path.join(path, "meta.json"))


class Shard:
    """Memory-mapped view of one split directory."""

    def __init__(self, path):
        with open(os.path.join(path, "meta.json")) as f:
            self.meta = json.load(f)
        if self.meta.get("format") != FORMAT or self.meta.get("version") != VERSION:
            raise ValueError(f"{path}: not a {FORMAT} v{VERSION} directory (meta.json says {self.meta})")
        self.path, self.n = path, int(self.meta["n"])
        self.image_codec = self.meta.get("image_codec", "raw")
        if self.image_codec not in CODECS:
            raise ValueError(f"{path}: unknown image_codec {self.image_codec!r}")
        ld = lambda name: np.load(os.path.join(path, name + ".npy"), mmap_mode="r")
        self.image_index = ld("image_index")
        self.images = np.memmap(os.path.join(path, "images.bin"), dtype=np.uint8, mode="r")
        self.barcode_offsets = ld("barcode_offsets")
        self.barcodes = np.memmap(os.path.join(path, "barcodes.bin"), dtype=np.uint8, mode="r")
        self.input_ids, self.token_type_ids, self.attention_mask = (ld(t) for t in _TEXT)
        self.processid, self.labels = ld("processid"), ld("labels")
        self.taxonomy = {t: ld(t) for t in _TAXA}
        self.image_nbytes = ld("image_bytes") if self.image_codec == "jpeg" else None
        self.image_ncoefs = ld("image_coefs") if self.image_codec == "jpeg" else None
        self.jpeg_sync_mcus = self.meta.get("jpeg_sync_mcus") if self.image_codec == "jpeg" else None
        self.image_sync = self.image_sync_offsets = None
        if self.jpeg_sync_mcus is not None:
            self.image_sync, self.image_sync_offsets = ld("image_sync"), ld("image_sync_offsets")
            if (len(self.image_sync_offsets) != self.n + 1 or self.image_sync.ndim != 2 or self.image_sync.shape[1] != 4
                    or int(self.image_sync_offsets[-1]) != len(self.image_sync)):
                raise ValueError(f"{path}: image_sync.npy / image_sync_offsets.npy disagree with n={self.n}")
        if self.image_nbytes is not None and len(self.image_nbytes) != self.n:
            raise ValueError(f"{path}: image_bytes.npy has {len(self.image_nbytes)} rows for n={self.n}")
        if not (len(self.image_index) == len(self.labels) == len(self.processid) == self.n and len(self.barcode_offsets) == self.n + 1):
            raise ValueError(f"{path}: array lengths disagree with meta.json n={self.n}")

    def __len__(self):
        return self.n

    def image(self, i):
        if self.image_codec != "raw":
            raise RuntimeError(f"{self.path}: a {self.image_codec} shard has no CPU decode path; read it through ShardLoader (the GPU "
                               "decodes), or take the stored stream with image_bytes(i)")
        off, h, w = (int(v) for v in self.image_index[i])
        return self.images[off:off + h * w * 3].reshape(h, w, 3)

    def image_bytes(self, i):
        """The stored JPEG stream of sample i (JPEG shards only)."""
        if self.image_codec != "jpeg":
            raise RuntimeError(f"{self.path}: a raw shard stores decoded pixels, not streams; use image(i)")
        off = int(self.image_index[i][0])
        return bytes(self.images[off:off + int(self.image_nbytes[i])])

    def barcode(self, i):
        return bytes(self.barcodes[int(self.barcode_offsets[i]):int(self.barcode_offsets[i + 1])]).decode("ascii")

    def label_dicts(self, idx):
        """The evaluation labels of ``get_array_of_label_dicts`` for the given samples."""
        return [{t: self.taxonomy[t][i].decode() for t in _TAXA} for i in idx]


LEVELS = _TAXA
EVAL_SPLITS = {"val": ("all_keys", "val_seen", "val_unseen"), "test": ("all_keys", "test_seen", "test_unseen")}


def eval_splits(root, which="val"):
    """The (keys, seen, unseen) shard directories of an evaluation root: a directory whose sub-directories are shards named after the
    reference's splits (dataset.py:371-530) -- ``all_keys`` and ``val_seen`` / ``val_unseen`` or ``test_seen`` / ``test_unseen``.
    Other sub-directories are ignored; a split that is absent or is not a shard raises ValueError."""
    if which not in EVAL_SPLITS:
        raise ValueError(f"eval split must be one of {tuple(EVAL_SPLITS)}, got {which!r}")
    paths = []
    for name in EVAL_SPLITS[which]:
        path = os.path.join(str(root), name)
        if not is_shard(path):
            raise ValueError(f"{root}: no shard for the split {name!r} (an evaluation root holds the shard directories "
                             f"{', '.join(EVAL_SPLITS[which])})")
        paths.append(path)
    return tuple(paths)


PROTOCOL_SPLITS = ("train_seen", "seen_keys", "val_unseen_keys", "test_unseen_keys", "val_seen", "val_unseen", "test_seen", "test_unseen")
NOT_A_CLASS = -1               # class index of a species outside the class list: the kernels' range checks flag it


def protocol_splits(root, names=PROTOCOL_SPLITS):
    """The shard directories ``names`` of a protocol root, in that order: a directory whose sub-directories are shards named after
    the splits of the reference's seen / unseen protocols (``PROTOCOL_SPLITS``).  The contract of ``eval_splits``: other
    sub-directories are ignored; a split that is absent or is not a shard raises ValueError."""
    names = tuple(names)
    unknown = [n for n in names if n not in PROTOCOL_SPLITS]
    if unknown:
        raise ValueError(f"protocol splits are {', '.join(PROTOCOL_SPLITS)}, got {unknown}")
    paths = []
    for name in names:
        path = os.path.join(str(root), name)
        if not is_shard(path):
            raise ValueError(f"{root}: no shard for the split {name!r} (a protocol root holds the shard directories "
                             f"{', '.join(names)})")
        paths.append(path)
    return tuple(paths)


def class_index_table(species_vocab, classes):
    """int32 ``[len(species_vocab)]``: species id (``taxonomy_ids``'s ``vocab["species"]`` order) -> its position in the class list
    ``classes`` as ``list.index`` gives it (the first occurrence of a repeated name), ``NOT_A_CLASS`` for a species that is not
    listed.  Host only, one pass over the two name lists; ``table[ids[:, species]]`` then is a whole split's class-index column."""
    first = {}
    for c, name in enumerate(classes):
        first.setdefault(name, c)
    return np.asarray([first.get(name, NOT_A_CLASS) for name in species_vocab], dtype=np.int32).reshape(-1)


def class_indices(ids, table, level=None):
    """The int32 ``[n]`` class-index column of one split: ``table`` (``class_index_table``) looked up with the split's species ids
    (``ids``: the int32 ``[n, L]`` array of ``taxonomy_ids`` -- its last column unless ``level`` says otherwise -- or ``[n]``)."""
    ids = np.asarray(ids)
    if ids.ndim == 2:
        ids = ids[:, -1 if level is None else level]
    return np.ascontiguousarray(np.asarray(table, dtype=np.int32)[ids])


def taxonomy_ids(shard_list, levels=LEVELS):
    """``hip/retrieval.encode_labels`` of the shards' ``label_dicts`` (every sample, in the given order) without building them:
    returns ``(arrays, vocab)``, one int32 ``[n, L]`` array per shard and ``vocab[level]`` = the names in id order.  Ids are handed
    out per level in order of first appearance over the shards in turn; equal strings get equal ids.  Works on the memory-mapped
    byte arrays with ``np.unique``: no Python loop over samples."""
    shard_list = [Shard(s) if isinstance(s, str) else s for s in shard_list]
    levels = list(levels)
    counts = [len(s) for s in shard_list]
    ids = np.empty((sum(counts), len(levels)), dtype=np.int32)
    vocab = {}
    for j, lv in enumerate(levels):
        names = np.concatenate([np.asarray(s.taxonomy[lv]) for s in shard_list]) if shard_list else np.zeros(0, dtype="S1")
        uniq, first, inverse = np.unique(names, return_index=True, return_inverse=True)
        order = np.argsort(first, kind="stable")            # the distinct names in order of first appearance
        rank = np.empty(len(uniq), dtype=np.int32)
        rank[order] = np.arange(len(uniq), dtype=np.int32)
        ids[:, j] = rank[inverse.reshape(-1)]
        vocab[lv] = [v.decode() for v in uniq[order].tolist()]
    bounds = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return [np.ascontiguousarray(ids[bounds[i]:bounds[i + 1]]) for i in range(len(shard_list))], vocab


class _Range(torch.utils.data.Dataset):
    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return i


def rank_indices(n, rank, world_size, shuffle, seed, epoch):
    """The sample order of the reference's ``prepare()`` for one rank and epoch: torch's own DistributedSampler with
    ``drop_last=True`` (dataset.py:42)."""
    sampler = torch.utils.data.DistributedSampler(_Range(n), num_replicas=world_size, rank=rank, shuffle=shuffle, seed=seed,
                                                  drop_last=True)
    sampler.set_epoch(epoch)
    return list(iter(sampler))


class ShardLoader:
    """Iterable over one split; see the module docstring.  ``for_training`` selects the augmentation chain and index labels
    (dataset.py:135-144), otherwise Resize -> CenterCrop and the taxonomy dictionaries as labels."""

    SLOTS = 3

    def __init__(self, shard, batch_size, rank=0, world_size=1, shuffle=False, seed=0, for_training=True, with_text=True,
                 device="cuda", augment_seed=None, decode_threads=4, entropy="host", labels=None):
        """``labels`` (slot 6 of the yielded tuple): ``None`` keeps what ``for_training`` selects (the training index labels, or the
        taxonomy dictionaries); ``"ids"`` yields the batch's sample indices instead, int64 ``[B]`` on the device, and builds no label
        dictionaries -- for consumers that keep the split's labels as resident columns and index them (``last_indices`` as a tensor).
        ``decode_threads`` (1..16, JPEG shards only): loader threads that entropy-decode a batch side by side.
        ``entropy`` (JPEG shards): ``"host"`` Huffman-decodes on those threads; ``"gpu"`` sends the stored bytes up and decodes them
        on the device from the shard's sync index (``write_shard(jpeg_sync_mcus=...)`` / ``add_jpeg_sync_index``).  In GPU mode a
        stream or index damaged after the shard was written -- shards are validated when written, so nothing else -- is found by
        the device; the loader reads a batch's status words where it next synchronises on that batch's staging slot (before the
        slot is refilled, and at the end of the iteration), so the ``RuntimeError`` naming the shard and the samples can arrive
        up to ``SLOTS - 1`` batches after the damaged batch was yielded."""
        from bioscanclip.util.gpu_pipeline import GpuAugment
        self.shard = Shard(shard) if isinstance(shard, str) else shard
        self.decode_threads = int(decode_threads)
        if not 1 <= self.decode_threads <= MAX_DECODE_THREADS:   # a fixed bound, never the machine's CPU count: the box is shared
            raise ValueError(f"decode_threads must be in 1..{MAX_DECODE_THREADS}, got {decode_threads}")
        if entropy not in ENTROPY_MODES:
            raise ValueError(f"entropy must be one of {ENTROPY_MODES}, got {entropy!r}")
        if entropy == "gpu" and (self.shard.image_codec != "jpeg" or self.shard.image_sync is None):
            what = "a raw shard has no streams to decode" if self.shard.image_codec != "jpeg" else "this JPEG shard has no sync index"
            raise ValueError(f"{self.shard.path}: entropy='gpu' needs a JPEG shard with a sync index ({what}); write it with "
                             "write_shard(..., jpeg_sync_mcus=...) or index it in place with shards.add_jpeg_sync_index(path)")
        if labels not in LABEL_MODES:
            raise ValueError(f"labels must be one of {LABEL_MODES}, got {labels!r}")
        self.entropy, self.labels = entropy, labels
        self._pool = None
        if self.shard.image_codec == "jpeg" and self.decode_threads > 1 and entropy == "host":
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=self.decode_threads, thread_name_prefix="bsclip-jpeg")
        self.batch_size, self.rank, self.world_size = int(batch_size), rank, world_size
        self.shuffle, self.seed, self.epoch = shuffle, seed, 0
        self.for_training, self.with_text, self.device = for_training, with_text, torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.augment = GpuAugment(for_training=for_training, seed=(seed + 17 * rank) if augment_seed is None else augment_seed)
        self.stream = torch.cuda.Stream(device=self.device)
        self._slots = [dict(cap_img=0, cap_dna=0) for _ in range(self.SLOTS)]
        self.last_params = None      # the augmentation draws of the most recently yielded batch (tests replay them on the CPU oracle)
        self.last_indices = None

    def set_epoch(self, epoch):
        """``DistributedSampler.set_epoch``: a different shuffle per epoch (and the reference's behaviour when it is never called:
        the same order every epoch)."""
        self.epoch = int(epoch)

    def indices(self):
        return rank_indices(len(self.shard), self.rank, self.world_size, self.shuffle, self.seed, self.epoch)

    def __len__(self):
        n = len(self.indices())
        return (n + self.batch_size - 1) // self.batch_size

    # ------------------------------------------------------------------------------------------------ producer side
    def _stage(self, slot, idx):
        """Host half of one batch: gather the samples into the slot's pinned buffers and draw the augmentation parameters."""
        from bioscanclip.util.gpu_pipeline import _resized_size
        sh = self.shard
        rows = sh.image_index[np.asarray(idx)]
        nbytes = int((rows[:, 1] * rows[:, 2]).sum()) * 3
        dna_len = int(sum(int(sh.barcode_offsets[i + 1] - sh.barcode_offsets[i]) for i in idx))
        jpeg = sh.image_codec == "jpeg"
        if slot["cap_img"] < nbytes:
            slot["cap_img"] = int(nbytes * 1.25) + 4096
            if not jpeg:                            # a JPEG batch reaches the device as coefficients (_stage_jpeg), not as pixels
                slot["img_host"] = torch.empty(slot["cap_img"], dtype=torch.uint8).pin_memory()
            with torch.cuda.stream(self.stream):   # the staging buffer belongs to the stream that writes and reads it: a block
                # of the default stream's pool could still be in use by queued kernels of the training step
                slot["img_dev"] = torch.empty(slot["cap_img"], dtype=torch.uint8, device=self.device)
        if slot["cap_dna"] < dna_len + 1:
            slot["cap_dna"] = int(dna_len * 1.25) + 1024
            slot["dna_host"] = torch.empty(slot["cap_dna"], dtype=torch.uint8).pin_memory()
            with torch.cuda.stream(self.stream):
                slot["dna_dev"] = torch.empty(slot["cap_dna"], dtype=torch.uint8, device=self.device)
        dna_np = slot["dna_host"].numpy()
        img_np = None if jpeg else slot["img_host"].numpy()
        sizes, off, doffs = [], 0, [0]
        for (o, h, w), i in zip(rows, idx):
            nb = int(h) * int(w) * 3
            if not jpeg:
                img_np[off:off + nb] = sh.images[int(o):int(o) + nb]
            off += nb
            sizes.append((int(h), int(w)))
            b0, b1 = int(sh.barcode_offsets[i]), int(sh.barcode_offsets[i + 1])
            dna_np[doffs[-1]:doffs[-1] + (b1 - b0)] = sh.barcodes[b0:b1]
            doffs.append(doffs[-1] + (b1 - b0))
        sel = np.asarray(idx)
        B = len(idx)
        if "meta_host" not in slot:   # small per-batch arrays share one pinned block per slot, allocated once (pinning is a
            T = int(self.shard.meta["text_len"])   # driver call that can synchronise the device: never per batch)
            slot["meta_host"] = torch.empty((self.batch_size + 1) + self.batch_size + 3 * self.batch_size * T,
                                            dtype=torch.int64).pin_memory()
        mh, T = slot["meta_host"], int(sh.meta["text_len"])
        off_h = mh[:B + 1]
        off_h.copy_(torch.tensor(doffs, dtype=torch.int64))
        host = {"sizes": sizes, "nbytes": nbytes, "indices": idx, "dna_offsets": off_h, "n_dna": doffs[-1],
                "params": [self.augment.sample(*_resized_size(h, w, self.augment.resize_to)) for h, w in sizes],
                "processid": [p.decode() for p in sh.processid[sel]]}
        if self.for_training or self.labels == "ids":
            lab = mh[self.batch_size + 1:self.batch_size + 1 + B]
            lab.copy_(torch.from_numpy(np.ascontiguousarray(sel if self.labels == "ids" else sh.labels[sel], dtype=np.int64)))
            host["label"] = lab
        else:
            host["label"] = sh.label_dicts(idx)
        if self.with_text:
            base = 2 * self.batch_size + 1
            host["text"] = []
            for k, a in enumerate((sh.input_ids, sh.token_type_ids, sh.attention_mask)):
                t = mh[base + k * self.batch_size * T:base + k * self.batch_size * T + B * T].view(B, T)
                t.copy_(torch.from_numpy(np.ascontiguousarray(a[sel])))
                host["text"].append(t)
        if jpeg and self.entropy == "gpu":
            host.update(self._stage_jpeg_gpu(slot, idx, rows))
        elif jpeg:
            host["ncoef"] = self._stage_jpeg(slot, idx, rows)
        return host

    def _stage_jpeg(self, slot, idx, rows):
        """Entropy-decode the batch's streams into the slot's pinned coefficient buffer, tables and records (the serial part of a
        JPEG decode, ``decode_threads`` streams at a time; the GIL is released inside the library).  Returns the coefficient count."""
        from bioscanclip.hip import ops
        sh, B = self.shard, len(idx)
        spans = [(int(rows[k][0]), int(sh.image_nbytes[i])) for k, i in enumerate(idx)]
        chunks = [range(t, B, self.decode_threads) for t in range(min(self.decode_threads, B))]
        run = (lambda fn: list(self._pool.map(fn, chunks))) if self._pool is not None else (lambda fn: [fn(c) for c in chunks])
        counts = np.asarray(sh.image_ncoefs[np.asarray(idx)], dtype=np.int64)    # written with the shard: no parse before the decode
        coef_off = np.concatenate([[0], np.cumsum(counts)])       # every count is a multiple of 64: so is every offset
        ncoef = int(coef_off[-1])
        if slot.get("cap_coef", 0) < ncoef:
            slot["cap_coef"] = int(ncoef * 1.25) + 4096
            slot["coef_host"] = torch.empty(slot["cap_coef"], dtype=torch.int16).pin_memory()
            with torch.cuda.stream(self.stream):
                slot["coef_dev"] = torch.empty(slot["cap_coef"], dtype=torch.int16, device=self.device)
                slot["planes_dev"] = torch.empty(ops.jpeg_pixels_workspace_bytes(slot["cap_coef"]), dtype=torch.uint8, device=self.device)
        if "rec_host" not in slot:     # allocated once per slot, like meta_host
            slot["rec_host"] = torch.empty((self.batch_size, 16), dtype=torch.int32).pin_memory()
            slot["qtab_host"] = torch.empty((self.batch_size * 3, 64), dtype=torch.int16).pin_memory()
        base = sh.images.ctypes.data
        coef_p, rec_p, qtab_p = slot["coef_host"].data_ptr(), slot["rec_host"].data_ptr(), slot["qtab_host"].data_ptr()

        def decode(chunk):   # pass 2: each image into its own range of the pinned buffers
            for k in chunk:
                o, n = spans[k]
                try:
                    ops.jpeg_entropy_decode(base + o, n, coef_p + 2 * int(coef_off[k]), int(counts[k]), qtab_p + 384 * k, rec_p + 64 * k)
                except ops.JpegRefused as exc:
                    raise RuntimeError(f"{sh.path}: sample {idx[k]}: {exc}") from exc
        run(decode)
        self._place_records(slot["rec_host"].numpy()[:B], rows, coef_off, idx)
        return ncoef

    def _place_records(self, rec, rows, coef_off, idx):
        """The batch fields of the B records the library wrote: where each image's coefficients, pixels and tables are."""
        B = len(idx)
        if not (np.array_equal(rec[:, 5], rows[:, 1]) and np.array_equal(rec[:, 4], rows[:, 2])):
            raise RuntimeError(f"{self.shard.path}: image_index.npy disagrees with the streams' own sizes (samples {list(idx)})")
        pix_off = np.concatenate([[0], np.cumsum(rows[:, 1] * rows[:, 2] * 3)])[:B]
        for col, v in ((0, coef_off[:B]), (2, pix_off)):          # 64-bit offsets as two int32
            rec[:, col] = (v & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            rec[:, col + 1] = (v >> 32).astype(np.int32)
        rec[:, 9:12] += 3 * np.arange(B, dtype=np.int32)[:, None]   # image k's tables are slots 3k .. 3k + 2

    def _stage_jpeg_gpu(self, slot, idx, rows):
        """GPU entropy mode: copy the batch's streams back to back into the slot's pinned byte buffer, gather their sync-index
        entries and parse their headers into device-ready tables and records.  Nothing is decoded on the host."""
        from bioscanclip.hip import lib as _l, ops
        sh, B, bs = self.shard, len(idx), self.batch_size
        sel = np.asarray(idx)
        lens = np.asarray(sh.image_nbytes[sel], dtype=np.int64)
        byte_off = np.concatenate([[0], np.cumsum(lens)])
        e0 = np.asarray(sh.image_sync_offsets[sel], dtype=np.int64)
        ents = np.asarray(sh.image_sync_offsets[sel + 1], dtype=np.int64) - e0
        ent_off = np.concatenate([[0], np.cumsum(ents)])
        counts = np.asarray(sh.image_ncoefs[sel], dtype=np.int64)
        coef_off = np.concatenate([[0], np.cumsum(counts)])
        ncoef, nbytes, nsync = int(coef_off[-1]), int(byte_off[-1]), int(ent_off[-1])
        with torch.cuda.stream(self.stream):
            if slot.get("cap_coef", 0) < ncoef:
                slot["cap_coef"] = int(ncoef * 1.25) + 4096
                slot["coef_dev"] = torch.empty(slot["cap_coef"], dtype=torch.int16, device=self.device)
                slot["planes_dev"] = torch.empty(ops.jpeg_pixels_workspace_bytes(slot["cap_coef"]), dtype=torch.uint8, device=self.device)
            if slot.get("cap_bytes", 0) < nbytes:
                slot["cap_bytes"] = int(nbytes * 1.25) + 4096
                slot["bytes_host"] = torch.empty(slot["cap_bytes"], dtype=torch.uint8).pin_memory()
                slot["bytes_dev"] = torch.empty(slot["cap_bytes"], dtype=torch.uint8, device=self.device)
            if slot.get("cap_sync", 0) < nsync:
                slot["cap_sync"] = int(nsync * 1.25) + 64
                slot["sync_host"] = torch.empty((slot["cap_sync"], 4), dtype=torch.int32).pin_memory()
                slot["sync_dev"] = torch.empty((slot["cap_sync"], 4), dtype=torch.int32, device=self.device)
            if "huff_host" not in slot:     # allocated once per slot, like meta_host
                slot["rec_host"] = torch.empty((bs, _l.JPEG_REC), dtype=torch.int32).pin_memory()
                slot["seg_host"] = torch.zeros((bs, _l.JPEG_SEG_REC), dtype=torch.int32).pin_memory()
                slot["qtab_host"] = torch.empty((bs * 3, 64), dtype=torch.int16).pin_memory()
                slot["huff_host"] = torch.empty((bs, 4 * _l.JPEG_HUFF_BYTES), dtype=torch.uint8).pin_memory()
                slot["status_host"] = torch.zeros(bs, dtype=torch.int32).pin_memory()
                slot["huff_dev"] = torch.empty((bs, 4 * _l.JPEG_HUFF_BYTES), dtype=torch.uint8, device=self.device)
                slot["status_dev"] = torch.zeros(bs, dtype=torch.int32, device=self.device)
        bytes_np, sync_np = slot["bytes_host"].numpy(), slot["sync_host"].numpy()
        base = sh.images.ctypes.data
        huff_p, rec_p, qtab_p = slot["huff_host"].data_ptr(), slot["rec_host"].data_ptr(), slot["qtab_host"].data_ptr()
        for k in range(B):
            o, n = int(rows[k][0]), int(lens[k])
            bytes_np[byte_off[k]:byte_off[k] + n] = sh.images[o:o + n]
            sync_np[ent_off[k]:ent_off[k + 1]] = sh.image_sync[e0[k]:e0[k] + ents[k]]
            try:
                ops.jpeg_device_tables(base + o, n, huff_p + 4 * _l.JPEG_HUFF_BYTES * k, qtab_p + 384 * k, rec_p + 64 * k)
            except ops.JpegRefused as exc:
                raise RuntimeError(f"{sh.path}: sample {idx[k]}: {exc}") from exc
        seg = slot["seg_host"].numpy()[:B]
        seg[:, 0], seg[:, 1], seg[:, 2], seg[:, 3] = byte_off[:B], lens, ent_off[:B], ents
        seg[:, 4], seg[:, 5] = int(sh.jpeg_sync_mcus), np.arange(B)
        self._place_records(slot["rec_host"].numpy()[:B], rows, coef_off, idx)
        return {"ncoef": ncoef, "jpeg_bytes": nbytes, "jpeg_sync": nsync}

    def _check_status(self, slot):
        """GPU entropy mode: the status words of the batch this slot last held.  The caller has synchronised on the slot's event."""
        idx = slot.pop("status_idx", None)
        if idx is None:
            return
        st = slot["status_host"][:len(idx)].numpy()
        if st.any():
            bad = [int(i) for i, s in zip(idx, st) if s]
            raise RuntimeError(f"{self.shard.path}: the device found damaged JPEG bytes or sync-index entries in samples {bad} (status "
                               f"{[int(s) for s in st if s]}, BSCLIP_JPEG_SEG_* bits); the batch that held them was yielded up to "
                               f"{self.SLOTS - 1} batches ago")

    def _enqueue(self, slot, host):
        """Device half, on the loader's side stream: H2D copies + the two transforms; records the slot's ready event."""
        from bioscanclip.hip import ops
        B = len(host["sizes"])
        with torch.cuda.stream(self.stream):
            if "jpeg_bytes" in host:   # JPEG shard, GPU entropy: bytes, index and tables go up, the device decodes into coef_dev
                n, nb, ne = host["ncoef"], host["jpeg_bytes"], host["jpeg_sync"]
                slot["bytes_dev"][:nb].copy_(slot["bytes_host"][:nb], non_blocking=True)
                slot["sync_dev"][:ne].copy_(slot["sync_host"][:ne], non_blocking=True)
                slot["huff_dev"][:B].copy_(slot["huff_host"][:B], non_blocking=True)
                qtab_dev = slot["qtab_host"][:3 * B].to(self.device, non_blocking=True)
                rec_dev = torch.empty((B, 16), dtype=torch.int32, device=self.device)
                seg_dev = torch.empty((B, 8), dtype=torch.int32, device=self.device)
                ops.jpeg_entropy_device(slot["bytes_dev"], slot["sync_dev"], slot["huff_dev"][:B], slot["rec_host"][:B], slot["seg_host"][:B],
                                        rec_dev, seg_dev, B, slot["coef_dev"], n, slot["status_dev"][:B])
                slot["status_host"][:B].copy_(slot["status_dev"][:B], non_blocking=True)   # read once the slot's event has passed
                slot["status_idx"] = list(host["indices"])
                ops.jpeg_pixels(slot["coef_dev"], n, qtab_dev, slot["rec_host"][:B], rec_dev, B, slot["planes_dev"], slot["img_dev"])
            elif "ncoef" in host:    # JPEG shard: coefficients, tables and records go up, the pixels are made in img_dev
                n = host["ncoef"]
                slot["coef_dev"][:n].copy_(slot["coef_host"][:n], non_blocking=True)
                qtab_dev = slot["qtab_host"][:3 * B].to(self.device, non_blocking=True)
                rec_dev = torch.empty((B, 16), dtype=torch.int32, device=self.device)    # filled by the library from rec_host
                ops.jpeg_pixels(slot["coef_dev"], n, qtab_dev, slot["rec_host"][:B], rec_dev, B, slot["planes_dev"], slot["img_dev"])
            else:
                slot["img_dev"][:host["nbytes"]].copy_(slot["img_host"][:host["nbytes"]], non_blocking=True)
            n_dna = host["n_dna"]
            slot["dna_dev"][:max(n_dna, 1)].copy_(slot["dna_host"][:max(n_dna, 1)], non_blocking=True)
            off_dev = host["dna_offsets"].to(self.device, non_blocking=True)
            image, _ = self.augment.run_packed(slot["img_dev"], host["sizes"], host["params"], device=self.device)
            dna = torch.empty(B, 660 // 5 + 1, dtype=torch.int64, device=self.device)
            ops.kmer_tokenize(slot["dna_dev"], off_dev, B, 660, 5, dna)
            out = {"image": image, "dna": dna, "processid": host["processid"], "params": host["params"]}
            if self.with_text:
                out["text"] = [t.to(self.device, non_blocking=True) for t in host["text"]]
            else:
                out["text"] = [None, None, None]
            out["label"] = host["label"].to(self.device, non_blocking=True) if torch.is_tensor(host["label"]) else host["label"]
            ev = torch.cuda.Event()
            ev.record(self.stream)
            out["ready"] = ev
        slot["out"] = out
        return out

    def __iter__(self):
        idx = self.indices()
        batches = [idx[i:i + self.batch_size] for i in range(0, len(idx), self.batch_size)]
        q = queue.Queue(maxsize=self.SLOTS - 1)
        dev = self.device

        def producer():
            cpu0 = time.thread_time()
            try:
                torch.cuda.set_device(dev)
                for k, b in enumerate(batches):
                    slot = self._slots[k % self.SLOTS]
                    if "out" in slot:
                        # the slot's pinned buffers are about to be refilled: its previous H2D copies (and the kernels that read
                        # its device staging buffers) must have run -- three batches ago, so this never waits in practice
                        slot["out"]["ready"].synchronize()
                        self._check_status(slot)
                    host = self._stage(slot, b)
                    q.put((k, b, self._enqueue(slot, host)))
                if self.entropy == "gpu":      # the last SLOTS batches: nothing refills their slots, so they are looked at here
                    for slot in self._slots:
                        if "status_idx" in slot:
                            slot["out"]["ready"].synchronize()
                            self._check_status(slot)
                q.put(None)
            except BaseException as exc:   # noqa: BLE001 - surface producer failures in the consumer
                q.put(exc)
            finally:
                self.producer_cpu_seconds = time.thread_time() - cpu0     # tools/jpeg_loader_bench.py reads it after th.join()

        th = threading.Thread(target=producer, daemon=True)
        th.start()
        while True:
            item = q.get()
            if item is None:
                break
            if isinstance(item, BaseException):
                raise item
            k, b, out = item
            cur = torch.cuda.current_stream(dev)
            cur.wait_event(out["ready"])
            for t in (out["image"], out["dna"], out["label"], *[x for x in out["text"] if x is not None]):
                if torch.is_tensor(t):       # every tensor allocated on the loader's stream and consumed on the caller's
                    t.record_stream(cur)
            self.last_params, self.last_indices = out["params"], b
            yield (out["processid"], out["image"], out["dna"], out["text"][0], out["text"][1], out["text"][2], out["label"])
        th.join()

    def __del__(self):
        pool = getattr(self, "_pool", None)
        if pool is not None:
            pool.shutdown(wait=False)


def convert_hdf5_split(hdf5_path, split, out_dir, dataset="bioscan_1m", labels=None, image_codec="raw", reencode=False,
                       jpeg_sync_mcus=None):
    """Write one split of the reference's HDF5 file (DATA.md:23-35; datasets image / image_mask / barcode /
    language_tokens_* / processid | image_file / order / family / genus / species, read as ``Dataset_for_CL`` reads them,
    dataset.py:219-265) as a shard directory.  Needs h5py, which this image does not have: run it where the data lives.
    ``image_codec="raw"`` decodes every image with Pillow; ``"jpeg"`` copies the stored streams (no Pillow) after checking that the
    loader's decoder takes each one.  Streams it does not take raise (``write_shard`` names the first ten) -- or, with ``reencode=True``, are
    re-encoded through Pillow as baseline 4:4:4 quality 95 and counted in meta.json ("reencoded").  ``jpeg_sync_mcus`` goes to
    ``write_shard``: the sync index for ``ShardLoader(entropy="gpu")``."""
    try:
        import io
        import h5py
    except ImportError as exc:   # pragma: no cover - the package does not exist in this image
        raise ImportError("convert_hdf5_split needs h5py (absent from the build image); run it on the data host") from exc
    g = h5py.File(hdf5_path, "r", libver="latest")[split]                     # pragma: no cover
    n = len(g["barcode"])                                                     # pragma: no cover
    pid_key = "processid" if dataset == "bioscan_5m" else "image_file"        # pragma: no cover
    stream = lambda i: g["image"][i].astype(np.uint8)[:g["image_mask"][i]].tobytes()   # pragma: no cover
    extra = {"reencoded": 0}                                                                # pragma: no cover

    def pixels():                                                             # pragma: no cover
        from PIL import Image
        for i in range(n):
            yield np.asarray(Image.open(io.BytesIO(stream(i))).convert("RGB"), dtype=np.uint8)

    def streams():                                                            # pragma: no cover
        for i in range(n):
            data = stream(i)
            try:
                _check_jpeg(data, i)
            except ValueError:
                from PIL import Image
                buf = io.BytesIO()
                Image.open(io.BytesIO(data)).convert("RGB").save(buf, format="JPEG", quality=95, subsampling="4:4:4")
                data = buf.getvalue()
                extra["reencoded"] += 1
            yield data

    images = pixels() if image_codec == "raw" else (stream(i) for i in range(n)) if not reencode else streams()   # pragma: no cover
    write_shard(out_dir, images, [b.decode("utf-8") for b in g["barcode"][:]],                           # pragma: no cover
                g["language_tokens_input_ids"][:], g["language_tokens_token_type_ids"][:], g["language_tokens_attention_mask"][:],
                [p.decode("utf-8") for p in g[pid_key][:]], labels=labels,
                taxonomy={t: [v.decode("utf-8") for v in g[t][:]] for t in _TAXA}, split=split, dataset=dataset,
                image_codec=image_codec, jpeg_sync_mcus=jpeg_sync_mcus)
    if image_codec == "jpeg" and reencode:                                    # pragma: no cover
        with open(os.path.join(out_dir, "meta.json")) as f:
            meta = json.load(f)
        meta.update(extra)
        with open(os.path.join(out_dir, "meta.json"), "w") as f:
            json.dump(meta, f)
