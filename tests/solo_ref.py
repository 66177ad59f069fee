"""The detector head's rule (Solov2::GetSegTensor, det2d/solo_head.cpp:410-559, with Solov2::MatrixNMS, :31-71) written with CPU torch from the reference's lines,
parameterised by dtype — float32 is what the reference runs, float64 is the yardstick — and an input generator that keeps the reference's own decisions away from rounding:

  dyadic inputs    mask features are multiples of 1/4 in [-1, 1] and kernel rows hold -1 / 0 / 1, so every product is a multiple of 1/4 and every logit is exact in
                   float32 in any summation order;
  no zero logit    the last feature channel is the constant 1 and its coefficient an odd multiple of 1/8: every logit is an odd multiple of 1/8;
  spaced scores    the category scores are chosen so that, IN THE FLOAT64 REFERENCE, consecutive sorted scores of both sorts differ by at least 1e-3 relative and no
                   score lies within 1e-3 relative of update_thr (asserted here).

No file outside the repository is read."""
import math

import numpy as np
import torch
import torch.nn.functional as F

SPACING = 1e-3


def floor_of_cells(n_cells, num_grids, strides, dtype):
    """strides = ones(kPredNum); slices up to the cumulative sums of num_grids^2 overwritten (solo_head.cpp:24-28,454-463)"""
    st = torch.ones(n_cells, dtype=dtype)
    cum = torch.tensor([float(g) for g in num_grids], dtype=torch.float32).pow(2).cumsum(0)
    st[: int(cum[0])] = strides[0]
    for i in range(1, len(num_grids)):
        st[int(cum[i - 1]): int(cum[i])] = strides[i]
    return st


def matrix_nms(seg_masks, cate_labels, cate_scores, sum_mask, kernel, sigma):
    n = cate_labels.shape[0]
    seg_masks = seg_masks.reshape(n, -1).to(cate_scores.dtype)
    inter = torch.mm(seg_masks, seg_masks.transpose(1, 0))
    sx = sum_mask.expand(n, n)
    iou = (inter / (sx + sx.transpose(1, 0) - inter)).triu(1)
    lx = cate_labels.expand(n, n)
    label = (lx == lx.transpose(1, 0)).to(cate_scores.dtype).triu(1)
    comp = (iou * label).max(0)[0]
    comp = comp.expand(n, n).transpose(1, 0)
    decay_iou = iou * label
    if kernel == "gaussian":
        coef = (torch.exp(-1 * sigma * decay_iou.pow(2)) / torch.exp(-1 * sigma * comp.pow(2))).min(0)[0]
    else:
        coef = ((1 - decay_iou) / (1 - comp)).min(0)[0]
    return cate_scores * coef


def head(kernels, cates, feature, par, dtype, stable=False):
    """GetSegTensor up to the second sort -> dict; every early return gives n = 0.  Inputs: numpy arrays or torch tensors; par["device"] (default "cpu") is where torch
    evaluates it (tests/tools/solo_head_cost.py runs these same lines on the GPU).  stable = True makes both sorts stable — equal scores stay in candidate order, then in
    first-sort order: the library's documented tie rule, which the reference's own unstable sort leaves open (the tie cases of tests/solo_cases.py)"""
    dev, lean = par.get("device", "cpu"), bool(par.get("lean"))          # lean: none of the diagnostic downloads below (the cost tool's timed runs)
    as_t = lambda a: (a if torch.is_tensor(a) else torch.from_numpy(a)).to(dev, dtype)
    C = feature.shape[0]
    kt = torch.cat([as_t(k).reshape(C, -1).permute(1, 0) for k in kernels], 0)
    ct = torch.cat([as_t(c).reshape(c.shape[0], -1).permute(1, 0) for c in cates], 0)
    feat = as_t(feature)
    out = dict(n=0, n_pass=0, n_floor=0, n_sorted=0)
    inds = ct > par["score_thr"]
    out["n_pass"] = int(inds.sum())
    if out["n_pass"] == 0:
        return out
    cate = ct.masked_select(inds)
    nz = inds.nonzero()
    labels, pred = nz[:, 1], nz[:, 0]
    kp = kt[pred]
    strides = floor_of_cells(ct.shape[0], par["num_grids"], par["strides"], dtype).to(dev)[pred]
    seg = F.conv2d(feat.unsqueeze(0), kp.view(kp.shape[0], kp.shape[1], 1, 1)).squeeze(0)
    out["logits"] = seg.clone() if dev == "cpu" and not lean else None
    seg = seg.sigmoid()
    masks = seg > par["mask_thr"]
    sums = masks.sum((1, 2)).to(dtype)
    keep = sums > strides
    if not lean:
        out["cand"] = (pred.cpu().numpy().copy(), labels.cpu().numpy().copy())
    out["n_floor"] = int(keep.sum())
    if out["n_floor"] == 0:
        return out
    cand_idx = torch.arange(cate.shape[0], device=dev)[keep]
    masks, seg, sums, cate, labels = masks[keep], seg[keep], sums[keep], cate[keep], labels[keep]
    if not lean:
        out["seg_scores"] = (((seg * masks.to(dtype)).sum((1, 2)) / sums).cpu(), cand_idx.cpu())
    cate = cate * ((seg * masks.to(dtype)).sum((1, 2)) / sums)
    order = torch.argsort(cate, dim=-1, descending=True, stable=stable)[: par["nms_pre"]]
    masks, seg, sums, cate, labels, cand_idx = masks[order], seg[order], sums[order], cate[order], labels[order], cand_idx[order]
    if not lean:
        out["sorted"] = (cand_idx.cpu().numpy().copy(), cate.cpu().numpy().copy())
    out["n_sorted"] = len(order)
    scores = matrix_nms(masks, labels, cate, sums, par["nms_kernel"], par["nms_sigma"])
    if not lean:
        out["updated"] = scores.cpu().numpy().copy()
    keep = scores >= par["update_thr"]
    if int(keep.sum()) == 0:
        return out
    seg, scores, labels, cand_idx = seg[keep], scores[keep], labels[keep], cand_idx[keep]
    order = torch.argsort(scores, dim=-1, descending=True, stable=stable)[: par["max_per_img"]]
    out.update(n=len(order), seg=seg[order], scores=scores[order].cpu().numpy().copy(), labels=labels[order].cpu().numpy().astype(np.int32), survivors=cand_idx[order].cpu().numpy().copy())
    return out


def resample(seg, par):
    """the two interpolations and the crop (solo_head.cpp:540-552) -> values [n, origin_h, origin_w] before the last threshold"""
    fh, fw = seg.shape[1:]
    x, y, w, h = par["rect"]
    v = F.interpolate(seg.unsqueeze(0), size=(fh * 4, fw * 4), mode="bilinear", align_corners=True)
    v = v[..., y: y + h, x: x + w]
    v = F.interpolate(v, size=(par["origin"][1], par["origin"][0]), mode="bilinear", align_corners=True)
    return v.squeeze(0)


def reference(inp, par, dtype, stable=False):
    out = head(inp["kernels"], inp["cates"], inp["feature"], par, dtype, stable)
    if out["n"]:
        out["values"] = resample(out["seg"], par).cpu().numpy()
        out["planes"] = out["values"] > par["mask_thr"]
    return out


def params(**kw):
    p = dict(score_thr=0.1, mask_thr=0.5, update_thr=0.05, nms_pre=48, max_per_img=8, nms_kernel="gaussian", nms_sigma=2.0, num_grids=(2, 2, 3, 4, 5), strides=(8, 8, 8, 8, 8),
             max_candidates=72, rect=(0, 0, 0, 0), origin=(0, 0))
    p.update(kw)
    return p


def relative_gaps(v):
    v = np.asarray(v, np.float64)
    v = np.sort(v[v > 0])[::-1]          # (a score the decay took to 0 lies under every threshold and is never sorted against a survivor)
    return np.inf if len(v) < 2 else float(np.min((v[:-1] - v[1:]) / np.abs(v[:-1])))


def make_case(channels, fh, fw, grids, n_classes, n_cand, n_surv, par, seed):
    """-> (inputs, par with update_thr placed, float64 head).  n_cand cells x classes pass score_thr; n_surv survive the second filter (clipped by what the pixel floor and
    nms_pre leave; 0 = keep update_thr as given).  The spacing conditions of the module's docstring are asserted on the float64 reference."""
    par = dict(par)
    for attempt in range(400):
        rng = np.random.default_rng(seed * 1000 + attempt)
        # smooth-ish dyadic features: a few random rectangles per channel, so that masks are blobs of many sizes
        feat = np.zeros((channels, fh, fw), np.float32)
        for c in range(channels - 1):
            feat[c] = rng.integers(-1, 2) / 4
            for _ in range(3):
                y0, x0 = int(rng.integers(0, fh)), int(rng.integers(0, fw))
                feat[c, y0: y0 + int(rng.integers(1, fh + 1)), x0: x0 + int(rng.integers(1, fw + 1))] = rng.integers(-4, 5) / 4
        feat[channels - 1] = 1.0
        kernels, cates = [], []
        for g in grids:
            k = rng.integers(-1, 2, (channels, g, g)).astype(np.float32) * (rng.random((channels, g, g)) < 6.0 / channels)
            k[channels - 1] = (2 * rng.integers(-2, 4, (g, g)) + 1) / 8
            kernels.append(np.ascontiguousarray(k, np.float32))
            cates.append(np.full((n_classes, g, g), 0.01, np.float32))
        n_cells = sum(g * g for g in grids)
        slots = rng.choice(n_cells * n_classes, n_cand, replace=False)
        slots.sort()
        level_off = np.cumsum([0] + [g * g for g in grids])

        def put(values):
            for s, v in zip(slots, values):
                cell, cls = divmod(int(s), n_classes)
                l = int(np.searchsorted(level_off, cell, side="right") - 1)
                cates[l].reshape(n_classes, -1)[cls, cell - level_off[l]] = v
        put(np.full(n_cand, 0.5))
        inp = dict(kernels=kernels, cates=cates, feature=feat)
        probe = dict(par, update_thr=0.0)
        h = head(kernels, cates, feat, probe, torch.float64)
        assert h["n_pass"] == n_cand
        assert not (h["logits"] == 0).any(), "a zero logit: the generator is wrong"
        # first-sort scores on a geometric grid (ratio 1.02), dealt at random; candidates under the pixel floor get the grid's low end
        target = 0.2 * 1.02 ** rng.permutation(n_cand)
        cate = np.full(n_cand, 0.15)
        if h["n_floor"]:
            ss, idx = h["seg_scores"]
            cate[idx.numpy()] = target[idx.numpy()] / ss.numpy()
        put(cate.astype(np.float32))
        h = head(kernels, cates, feat, probe, torch.float64)
        if h["n_pass"] != n_cand:
            continue
        if h["n_floor"] == 0:
            if n_surv == 0:
                return inp, par, h
            continue
        upd = np.sort(h["updated"])[::-1]
        if relative_gaps(h["sorted"][1]) < SPACING or relative_gaps(upd) < SPACING:
            continue
        if n_surv:
            k = min(n_surv, len(upd))
            lo = upd[k] if k < len(upd) else upd[k - 1] * 0.5
            par["update_thr"] = float(np.float32(math.sqrt(upd[k - 1] * lo)))
        thr = par["update_thr"]
        if np.min(np.abs(upd - thr)) < SPACING * thr:
            continue
        h = head(kernels, cates, feat, par, torch.float64)
        assert relative_gaps(h["sorted"][1]) >= SPACING and relative_gaps(h["updated"][h["updated"] >= thr]) >= SPACING
        return inp, par, h
    raise AssertionError("no input with spaced scores found")
