#!/usr/bin/env python3
"""Makes tests/golden/match_feature_image.npz: the image the reference's test/test-match-feature.py matches in,
test/data/figueroa-overpass-looking-S.0.downsampled.jpg, decoded to grayscale with PIL: one (482, 722) uint8 array,
'image'. The tests read the array only; this script runs where /root/reference exists.

    python3 tests/golden/make_match_feature_image.py
"""
import os
import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
SRC  = "/root/reference/test/data/figueroa-overpass-looking-S.0.downsampled.jpg"

image = np.asarray(Image.open(SRC).convert('L'))
assert image.dtype == np.uint8 and image.shape == (482, 722), (image.dtype, image.shape)
out = os.path.join(HERE, "match_feature_image.npz")
np.savez_compressed(out, image=image)
assert np.array_equal(np.load(out)["image"], image)
print(out, os.path.getsize(out), "bytes;", image.shape, image.dtype)
