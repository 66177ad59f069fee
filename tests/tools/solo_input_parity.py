"""The observed distances behind tests/test_solo_input.py and tests/test_solo_input_ref.py, per image x model pair: the largest |device - restatement| and
|CPU torch - restatement| (tests/solo_input_ref.py; the bar is 2e-6, derived there), and how many rectangle elements of a constant-colour image the device leaves off
the constant.  Writes profiles/solo_input_parity.json.

    python tests/tools/solo_input_parity.py
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    import torch
    assert torch.cuda.is_available(), "needs a GPU"
    from dynamic_vins_amd.frontend import Context, make_cam
    from tests import solo_input_ref as sr
    from tests.test_solo_input_ref import PAIRS
    recs = []
    for (w, h), (mw, mh) in PAIRS:
        _, img = sr.image(w, h, seed=w + h)
        r = sr.solo_input(img, mw, mh)
        cam = make_cam(100, 100, w / 2, h / 2)
        ctx = Context(width=w, height=h, max_cnt=50, min_dist=10, cam0=cam, cam1=cam)
        dev = ctx.solo_input(np.ascontiguousarray(img), mw, mh)[0].cpu().numpy()
        x, y, rw, rh = r["rect"]
        off = {}
        for col in ((0, 0, 0), (255, 255, 255), (17, 130, 201)):
            flat = np.empty((h, w, 3), np.uint8)
            flat[:] = col
            got = ctx.solo_input(flat, mw, mh)[0].cpu().numpy()[:, y:y + rh, x:x + rw]
            const = sr.normalise(flat)[:, 0, 0]
            off["%d,%d,%d" % col] = [int((got[c].view(np.uint32) != const[c].view(np.uint32)).sum()) for c in range(3)]
        ctx.close()
        recs.append(dict(image=[w, h], model=[mw, mh], rect=list(r["rect"]), device_minus_restatement=float(np.abs(dev.astype(np.float64) - r["out"]).max()),
                         torch_minus_restatement=float(np.abs(sr.torch_reference(img, mw, mh).astype(np.float64) - r["out"]).max()),
                         constant_colour_elements_off_per_plane=off, rect_elements_per_plane=rw * rh))
        print(recs[-1])
    with open(os.path.join(ROOT, "profiles", "solo_input_parity.json"), "w") as f:
        json.dump(dict(what="largest absolute distance to tests/solo_input_ref.py (float32 weights, float64 interpolation sum) on random bytes; bar 2e-6", bar=sr.BAR, records=recs), f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
