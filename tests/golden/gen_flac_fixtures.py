"""Copies four of the reference's own recorded FLAC files (real libFLAC streams: LPC, Rice2, 4096- and 1024-sample
frames) to tests/golden/flac/.  Runs only where the reference checkout exists:

    python tests/golden/gen_flac_fixtures.py /path/to/reference
"""
import os
import shutil
import sys

FILES = ('short_window_demo/6/sw_6_26.flac', 'short_window_demo/10/sw_10_29.flac', 'short_window_demo/8/sw_8_85.flac',
         'short_window_demo/8/sw_8_39.flac')

if __name__ == '__main__':
    ref = sys.argv[1]
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'flac')
    os.makedirs(out, exist_ok=True)
    for f in FILES:
        assert os.path.getsize(os.path.join(ref, f)) < 32 * 1024, f
        shutil.copyfile(os.path.join(ref, f), os.path.join(out, os.path.basename(f)))
        print(f)
