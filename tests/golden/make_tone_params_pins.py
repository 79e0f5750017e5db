"""Generate tests/golden/tone_params_pins.json by executing the REFERENCE's own shader text over the table of tests/tone_params.py.

Runs only where the reference tree is mounted and oracle/_ref is built.  For every case of tone_params.pin_cases() (the designed 256 x 32
frame through every HDR10 / Dolby Vision row x six operators of ps_hdr10_tonemap.hlsl, same size and 1.5x; through the PQ -> SDR and
HLG -> SDR convert shader at every SDR_NITS value, same size and 2x) the whole Process() is run through oracle/ref_hlsl and recorded:
  * sha256 of the B, G, R channels of the render target;
  * the settings of the case.  No pixel is stored; how the oracle compares is printed, and tests/test_tone_params.py holds it to the hashes.

    python tests/golden/make_tone_params_pins.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_hlsl"))
from oracle import oracle as O  # noqa: E402
import ref_pipeline as RP  # noqa: E402
from tests import tone_params as T  # noqa: E402
from tests.golden import cases  # noqa: E402
from tests.golden.make_ref_hlsl_golden import rgb_channels  # noqa: E402


def run_pair(c, frame, pitch):
    p = cases.oracle_params(O, c)
    a = O.process(p, frame, pitch)
    b = RP.process(p, frame, pitch)
    if b.ndim == 2:
        a = a.view(np.uint32).reshape(b.shape)
    return rgb_channels(a), rgb_channels(b)


def main():
    frame, pitch = T.frame()
    pins, worst = {}, 0
    for key, c in T.pin_cases().items():
        ca, cb = run_pair(c, frame, pitch)
        d = np.abs(ca - cb)
        pins[key] = dict(rgb_sha256=hashlib.sha256(cb.astype(np.uint16).tobytes()).hexdigest(), case=T.describe(c))
        worst = max(worst, int(d.max()))
        print(f"{key:55s} max {d.max()} differing {100 * (d > 0).mean():.4f}%")
    with open(os.path.join(HERE, "tone_params_pins.json"), "w") as f:
        json.dump(dict(source="reference HLSL text executed by oracle/ref_hlsl over tests/tone_params.py (frame(), HDR10_ROWS, DOVI_ROWS, SDR_NITS)",
                       frame_sha256=hashlib.sha256(frame.tobytes()).hexdigest(), cases=pins), f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    print(f"{len(pins)} cases, oracle worst {worst}")


if __name__ == "__main__":
    main()
