#!/usr/bin/env python3
"""Records tests/golden/png_sizes.json: on the level images of the recordings tests/test_png_cpu.py lists, the bytes of
the PNG rule's IDAT payloads (tests/png_reference.py), of zlib's Z_RLE strategy on the same filtered bytes, and their
ratio -- the bar of test_compression_stays_within_two_hundredths_of_zlib_rle is that ratio plus 0.02.

    python tests/golden/gen_png_sizes.py
"""
import json
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), 'amt-saga_amd'))
import png_reference as R            # noqa: E402
import test_png_cpu as T             # noqa: E402

waves = np.load(os.path.join(HERE, 'recorded_waves.npz'))
rows, ours, rle, raw = {}, 0, 0, 0
for key in T.RECORDINGS:
    info = {}
    R.encode(T.spectrogram_image(waves[key]), None, info)
    z = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    n_rle = len(z.compress(info['filtered']) + z.flush())
    rows[key] = dict(payload=info['payload'], z_rle=n_rle, zlib6=len(zlib.compress(info['filtered'], 6)),
                     filtered=len(info['filtered']), kinds=sorted(set(info['kinds'])))
    ours, rle, raw = ours + info['payload'], rle + n_rle, raw + len(info['filtered'])
out = dict(recordings=list(T.RECORDINGS), size=[T.IMAGE_W, T.IMAGE_H], payload=ours, z_rle=rle, filtered=raw,
           ratio=round(ours / rle, 4), per_recording=rows)
with open(os.path.join(HERE, 'png_sizes.json'), 'w') as f:
    json.dump(out, f, indent=1, sort_keys=True)
    f.write('\n')
print(json.dumps(out, indent=1, sort_keys=True))
