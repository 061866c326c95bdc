"""Write tests/golden/jpeg/: small JPEG files made with Pillow, Pillow's own decode of each (``Image.open(...).convert("RGB")``) as
.npy, and manifest.json.  The set is the smallest shapes at which each piece of the decoder can go wrong (sizes that are no MCU
multiple, every sampling mode Pillow writes, custom Huffman tables, restart markers, grey, coarse and unit quantisation, a content
that drives the clamp to 0 and 255) plus one progressive file that the decoder must refuse.  Needs Pillow; the tests read only
what this writes.

    python tools/make_jpeg_fixtures.py
"""
import io
import json
import os

import numpy as np
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "jpeg")

# name, W, H, mode, content, save options
CASES = [
    ("c8x8_444", 8, 8, "RGB", "smooth", dict(subsampling="4:4:4", quality=85)),
    ("c17x9_444_opt", 17, 9, "RGB", "smooth", dict(subsampling="4:4:4", quality=85, optimize=True)),
    ("c37x29_420_q75", 37, 29, "RGB", "smooth", dict(subsampling="4:2:0", quality=75)),
    ("c33x16_422_q50", 33, 16, "RGB", "smooth", dict(subsampling="4:2:2", quality=50)),
    ("c48x40_420_rst", 48, 40, "RGB", "smooth", dict(subsampling="4:2:0", quality=85, restart_marker_rows=1)),
    ("c20x20_grey", 20, 20, "L", "smooth", dict(quality=85)),
    ("c31x31_420_q10", 31, 31, "RGB", "contrast", dict(subsampling="4:2:0", quality=10)),
    ("c24x24_444_q100", 24, 24, "RGB", "smooth", dict(subsampling="4:4:4", quality=100)),
    ("c64x48_420_q90", 64, 48, "RGB", "smooth", dict(subsampling="4:2:0", quality=90)),
    # Pillow writes no 4:4:0.  A 4:2:2 stream of 28 x 44 has 2 x 6 MCUs of [Y Y Cb Cr]; with the luma factors in its frame header
    # swapped from 2x1 to 1x2 the same bytes are a valid 4:4:0 stream of 4 x 3 MCUs: the picture is scrambled, the decode is defined
    ("c28x44_440_patched", 28, 44, "RGB", "smooth", dict(subsampling="4:2:2", quality=80, patch_440=True)),
]
REFUSED = [("p16x16_progressive", 16, 16, "RGB", "smooth", dict(subsampling="4:2:0", quality=85, progressive=True))]


def content(kind, w, h, channels, rng):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    if kind == "contrast":     # saturated checker blocks + strong noise: coarse quantisation overshoots past 0 and 255
        base = np.where(((x // 5 + y // 3) % 2) > 0, 255.0, 0.0)[..., None].repeat(channels, axis=2)
        base[..., 0 % channels] = np.where((x // 7) % 2 > 0, 255.0, 0.0)
        img = base + rng.normal(0, 40, size=(h, w, channels))
    else:                      # smooth gradients of different direction per channel + mild noise
        planes = [255 * x / max(w - 1, 1), 255 * y / max(h - 1, 1), 255 * (x + y) / max(w + h - 2, 1)]
        img = np.stack(planes[:channels], axis=2) + rng.normal(0, 6, size=(h, w, channels))
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    return img[..., 0] if channels == 1 else img


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20240607)
    manifest = {"decoded_by": "Pillow Image.open(...).convert('RGB')", "fixtures": [], "refused": []}
    for group, cases in (("fixtures", CASES), ("refused", REFUSED)):
        for name, w, h, mode, kind, opts in cases:
            img = content(kind, w, h, 1 if mode == "L" else 3, rng)
            buf = io.BytesIO()
            Image.fromarray(img, mode).save(buf, format="JPEG", **{k: v for k, v in opts.items() if k != "patch_440"})
            data = buf.getvalue()
            if opts.get("patch_440"):
                sof = data.index(b"\xff\xc0")
                assert data[sof + 11] == 0x21
                data = data[:sof + 11] + b"\x12" + data[sof + 12:]
            with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
                f.write(data)
            entry = {"name": name, "width": w, "height": h, "mode": mode, "content": kind, "bytes": len(data),
                     "options": {k: v for k, v in opts.items()}}
            if group == "fixtures":
                px = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)
                assert px.shape == (h, w, 3)
                np.save(os.path.join(OUT, name + ".npy"), px)
                entry["min"], entry["max"] = int(px.min()), int(px.max())
            manifest[group].append(entry)
            print(f"{name}: {len(data)} bytes")
    with open(os.path.join(OUT, "manifest.json"), "w") as f:
        json.dump(manifest, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
