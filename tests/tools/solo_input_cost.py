"""Cost of the detector's input stage at the reference's shapes: image 1242 x 375 into the 1152 x 384 network, the frame in device memory.  dv_solo_input_enqueue ->
_collect, wall clock, median of 20 with min and max, and next to it the same formulas — swap, (t - mean) / std, F.interpolate(bilinear, align_corners=True), zero cat, all
float32 — run by torch on the same GPU in the same process, alternating: what a port has today.  The largest |library - torch| of the last frame is recorded beside the
times.  Writes profiles/solo_input_cost.json.

    python tests/tools/solo_input_cost.py             # -> profiles/solo_input_cost.json
    python tests/tools/solo_input_cost.py --frames 5  # a short run that writes nothing (the command for a kernel trace)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H, MW, MH, REPS, WARM = 1242, 375, 1152, 384, 20, 3


def median(v):
    v = sorted(v)
    return 0.5 * (v[len(v) // 2 - 1] + v[len(v) // 2])


def run(reps):
    import numpy as np
    import torch
    import torch.nn.functional as F
    from dynamic_vins_amd.frontend import Context, DV_MEM_DEVICE, SOLO_IMG_MEAN, SOLO_IMG_STD, make_cam
    img = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8)).cuda()
    mean_t = torch.tensor(SOLO_IMG_MEAN, dtype=torch.float32, device="cuda").reshape(3, 1, 1).expand(3, H, W)
    std_t = torch.tensor(SOLO_IMG_STD, dtype=torch.float32, device="cuda").reshape(3, 1, 1).expand(3, H, W)
    torch.cuda.synchronize()
    ctx = Context(width=W, height=H, max_cnt=150, min_dist=30, cam0=make_cam(721.5, 721.5, 609.6, 172.9), cam1=make_cam(721.5, 721.5, 609.6, 172.9))
    t_lib, t_torch, diff = [], [], 0.0
    for _ in range(WARM + reps):
        t0 = time.perf_counter()
        ctx.solo_input_enqueue(img.data_ptr(), MW, MH, mem=DV_MEM_DEVICE, stride=img.stride(0))
        ptr, shape, rect = ctx.solo_input_collect()
        t_lib.append(time.perf_counter() - t0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t = img.to(torch.float32)
        t = torch.cat([t[..., 2].unsqueeze(2), t[..., 1].unsqueeze(2), t[..., 0].unsqueeze(2)], 2).permute(2, 0, 1)
        t = (t - mean_t) / std_t
        t = F.interpolate(t.unsqueeze(0), size=(rect[3], rect[2]), mode="bilinear", align_corners=True).squeeze(0)
        cat_t = torch.zeros(3, (MH - rect[3]) // 2, MW, dtype=torch.float32, device="cuda")
        t = torch.cat([cat_t, t, cat_t], 1).contiguous()
        torch.cuda.synchronize()
        t_torch.append(time.perf_counter() - t0)
    from dynamic_vins_amd.frontend import device_tensor
    diff = float((device_tensor(ptr, shape) - t).abs().max())
    ctx.close()
    t_lib, t_torch = t_lib[WARM:], t_torch[WARM:]
    return dict(reps=reps, rect=list(rect), library_ms=dict(median=1e3 * median(t_lib), min=1e3 * min(t_lib), max=1e3 * max(t_lib)),
                torch_same_gpu_ms=dict(median=1e3 * median(t_torch), min=1e3 * min(t_torch), max=1e3 * max(t_torch)), max_abs_library_minus_torch=diff)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "solo_input_cost.json"))
    a = ap.parse_args()
    rec = run(a.frames or REPS)
    print(rec)
    if a.frames:
        return 0
    out = dict(what="dv_solo_input_enqueue -> _collect against the same formulas in torch (float32) on the same GPU, alternating in one process; wall clock per frame; the frame "
                    "in device memory; the torch path ends with the contiguous padded tensor on the device and a synchronize",
               shape=dict(image=[W, H], model=[MW, MH]), unit="ms", record=rec,
               traffic_arithmetic=dict(note="bytes per frame, arithmetic, not measured", frame_in=3 * W * H, tensor_out=4 * 3 * MW * MH))
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
