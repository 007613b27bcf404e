#!/usr/bin/env python3
"""Golden vectors for the JPEG leg of save() (cv::imwrite(filename, result), MultiBandMap2DCPU.cpp:841: libjpeg at OpenCV 2.4.9's
defaults, 4:2:0, the quality given).  libjpeg is a third-party dependency that is not part of the reference tree, so the expected streams come from
libjpeg-turbo itself, through Pillow: save(..., "JPEG", quality=q, subsampling=2) writes the same marker sequence (JFIF 1.01, two DQT,
SOF0, four DHT, one SOS).  Only the streams are stored: the pictures are rebuilt from (rows, cols, kind) by tests/jpeg_encode_model.py.
    python tests/golden/make_jpeg_encode_vectors.py        -> tests/golden/jpeg_encode_vectors.npz
"""
import io
import json
import os
import sys

import numpy as np
from PIL import Image, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_encode_model as model  # noqa: E402


def main():
    arrays = {}
    for i, (h, w, kind, q) in enumerate(model.CASES):
        b = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(model.content(h, w, kind, i)[:, :, ::-1])).save(b, "JPEG", quality=q, subsampling=2)
        arrays["stream%02d" % i] = np.frombuffer(b.getvalue(), np.uint8)
    meta = {"cases": [list(c) for c in model.CASES], "libjpeg": features.version("jpg"), "pillow": features.version("pil")}
    arrays["meta"] = np.frombuffer(json.dumps(meta).encode(), np.uint8)
    out = os.path.join(HERE, "jpeg_encode_vectors.npz")
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes,", len(model.CASES), "cases")


if __name__ == "__main__":
    main()
