"""The reference's SHIPPED parameter sets (config/**.yaml) through the product.

CPU (`-m "not gpu"`; the shipped files are rebuilt from the values tests/golden/ref_config.json keeps of them — the keys the shim and these tests read):
  * every top-level YAML the reference ships is read by the C++ shim's ReadConfig (dynamic_vins_amd/host/dvins_shim.hpp) and either yields the values an
    independent Python read of the same file gives, or throws exactly where the reference's own Config / VioParameters constructors throw
    (utils/parameters.cpp:134-137, estimator/vio_parameters.cpp:54-61);
  * the tables of dynamic_vins_amd/ref_configs.py (what the GPU tests and bench.py run) equal the YAMLs they cite.

GPU (`-m gpu`): images -> trajectory parity against the oracle AT those parameter sets, from pixels, dynamic mode, objects in every frame:
  viode.yaml (752x480, 160 / 20, erosion 5, 8 iterations, VIO), zed_1280x720_vision_only/dynamic.yaml (1280x720, 400 / 25, erosion 20, 10 iterations,
  vision only, use_det3d 1, two different undistorted cameras), kitti_tracking_online.yaml (1242x375, dynamic + use_line 1 + plane_constraint 1:
  LinePoint + dynamic with detector segments through UndistortedLineEndPoints), and BASELINE.json config 5 as stated — the ZED set with use_line 1
  (1280x720 LinePoint + dynamic together).  Bars as in tests/test_dynamic_pipeline.py."""
import glob
import json
import os
import subprocess

import numpy as np
import pytest

from dynamic_vins_amd import ref_configs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DATA = os.path.join(ROOT, "tests", "golden", "ref_config.json")          # tests/golden/gen_golden.py ref_config
KITTI_CALIB = os.path.join(ROOT, "tests", "golden", "config", "kitti_calib") + "/"


@pytest.fixture(scope="module")
def shim_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("shimcfg") / "shim_test")
    lib = os.path.join(ROOT, "dynamic_vins_amd", "lib")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "dynamic_vins_amd", "host"),
           os.path.join(ROOT, "tests", "host", "shim_test.cpp"), "-o", exe, "-L" + lib, "-ldvins_hip", "-Wl,-rpath," + lib, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def ref_cfg(tmp_path_factory):
    """the reference's config/ tree rebuilt from tests/golden/ref_config.json: every shipped configuration file with the scalars and body_T_cam matrices the shim
    reads, the camera files they name, and a header-only stand-in for the label table a VIODE configuration points to (only its presence is read here)"""
    data = json.load(open(REF_DATA))
    root = tmp_path_factory.mktemp("ref")
    for rel, c in data["configs"].items():
        lines = ["%YAML:1.0", "---"] + ["%s: %s" % kv for kv in c["scalars"].items()]
        for k, m in c["matrices"].items():
            lines += ["%s: !!opencv-matrix" % k, "  rows: %d" % (len(m) // 4), "  cols: 4", "  dt: d", "  data: [%s]" % ", ".join(repr(float(x)) for x in m)]
        _write(root / "config" / rel, lines)
    for rel, c in data["cameras"].items():
        lines, sections = ["%YAML:1.0", "---"], {}
        for k, v in c.items():
            if "." in k:
                sections.setdefault(k.split(".", 1)[0], []).append("   %s: %s" % (k.split(".", 1)[1], v))
            else:
                lines.append("%s: %s" % (k, v))
        for sec, body in sections.items():
            lines += [sec + ":"] + body
        _write(root / "config" / rel, lines)
    for rel in data["label_files"]:
        _write(root / rel, ["label_id,r,g,b"])
    return str(root / "config")


def _write(path, lines):
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text("\n".join(lines) + "\n")


def shipped_yamls(ref_cfg):
    """the top-level configuration files (they name a slam_type); camera files and VIODE's own calibration dump are not configs"""
    out = []
    for f in sorted(glob.glob(os.path.join(ref_cfg, "**", "*.yaml"), recursive=True)):
        if "slam_type" in ref_configs.yaml_scalars(f):
            out.append(f)
    return out


def shim_config(exe, path):
    out = subprocess.run([exe, "config", path, "0000", KITTI_CALIB], capture_output=True, text=True, check=True).stdout
    if out.startswith("THROWN"):
        return out.strip()
    return dict(ln.split("=", 1) for ln in out.splitlines())


def test_estimate_extrinsic_and_td_keys_reach_the_estimator_config(shim_exe, tmp_path):
    """utils/parameters.cpp:82-99: estimate_extrinsic / estimate_td are read only with an IMU; 1 frees the blocks around the configured extrinsics (dv_est_config::estimate bit 0 / 1),
    estimate_extrinsic 2 (calibration without an initial guess) is refused by the shim"""
    import shutil
    src = os.path.join(ROOT, "tests", "golden", "config")
    for f in os.listdir(src):
        if os.path.isfile(os.path.join(src, f)):
            shutil.copy(os.path.join(src, f), tmp_path / f)
    base = open(os.path.join(src, "zed_like.yaml")).read()
    assert "estimate_extrinsic: 0" in base and "estimate_td: 0" in base and "\nimu: 1" in base
    for ex, td, imu, want in ((0, 0, 1, "0"), (1, 0, 1, "1"), (0, 1, 1, "2"), (1, 1, 1, "3"), (1, 1, 0, "0"), (2, 0, 1, None)):
        txt = base.replace("estimate_extrinsic: 0", "estimate_extrinsic: %d" % ex).replace("estimate_td: 0", "estimate_td: %d" % td).replace("\nimu: 1", "\nimu: %d" % imu)
        path = tmp_path / "zed_like.yaml"
        path.write_text(txt)
        c = shim_config(shim_exe, str(path))
        if want is None:
            assert isinstance(c, str) and "estimate_extrinsic 2" in c, c
        else:
            assert not isinstance(c, str), c
            assert c["estimate"] == want and c["use_imu"] == str(imu), (ex, td, imu, c["estimate"])


def test_every_shipped_yaml_constructs_the_shim_config(shim_exe, ref_cfg):
    files = shipped_yamls(ref_cfg)
    assert len(files) >= 14, files
    built, thrown = [], []
    for f in files:
        y = ref_configs.yaml_scalars(f)
        c = shim_config(shim_exe, f)
        st = y["slam_type"]
        dynamic = st not in ("raw", "naive")          # utils/parameters.cpp:29-36 (a numeric node reads as "" -> dynamic)
        if isinstance(c, str):
            # the only legitimate failures: a dynamic config without use_det3d / instance_init_min_num (the reference throws there too), or a camera model off the path
            assert dynamic and ("use_det3d" not in y or "instance_init_min_num" not in y) or "PINHOLE" in c, (f, c)
            thrown.append(os.path.relpath(f, ref_cfg))
            continue
        built.append(os.path.relpath(f, ref_cfg))
        assert c["dynamic"] == str(int(dynamic)) and c["naive"] == str(int(st == "naive")), f
        for key, ykey in [("width", "image_width"), ("height", "image_height"), ("max_cnt", "max_cnt"), ("min_dist", "min_dist"), ("max_iters", "max_num_iterations"),
                          ("use_imu", "imu"), ("use_line", "use_line"), ("plane_constraint", "plane_constraint")]:
            assert int(c[key]) == int(float(y.get(ykey, 0))), (f, key)
        assert float(c["keyframe_parallax"]) == float(y["keyframe_parallax"]), f
        morph = int(y.get("mask_morphology_size", 0)) if int(y.get("use_mask_morphology", 0)) else 0
        assert int(c["mask_morphology_size"]) == morph, f
        if int(y["imu"]):
            for k in ("acc_n", "gyr_n", "acc_w", "gyr_w", "g_norm"):
                assert float(c[k]) == float(y[k]), (f, k)
        if dynamic:
            assert int(c["use_det3d"]) == int(y["use_det3d"]) and int(c["min_dynamic_dist"]) == int(y["min_dynamic_dist"]) and int(c["max_dynamic_cnt"]) == int(y["max_dynamic_cnt"]), f
            assert float(c["static_inst_threshold"]) == float(y.get("static_inst_threshold", 10.0)), f
        assert c["every_frame"] == str(int(y["dataset_type"].lower() == "kitti")), f
        if y["dataset_type"].lower() == "kitti" and "kitti_calib_path" in y:
            assert [float(v) for v in c["cam0"].split()][:4] == [721.5377, 721.5377, 609.5593, 172.854], f            # P2 of the calib fixture
            assert abs(float(c["baseline"]) - (339.5242 + 44.85728) / 721.5377) < 1e-12 and c["tic1"].split()[0] == c["baseline"], f
            assert c["ric0"].split() == ["1", "0", "0", "0", "1", "0", "0", "0", "1"], f
    # all the configurations BASELINE.json's configs and SURVEY 8 name are among the ones that build
    for need in ("viode/viode.yaml", "euroc/euroc.yaml", "custom/zed_1280x720_vision_only/dynamic.yaml", "custom/zed_1280x720/custom.yaml",
                 "kitti/kitti_tracking/kitti_tracking.yaml", "kitti/kitti_tracking/kitti_tracking_online.yaml"):
        assert need in built, (need, thrown)


def test_tables_match_the_shipped_yamls(ref_cfg):
    for name, c in ref_configs.CONFIGS.items():
        path = os.path.join(ref_cfg, c["yaml"])
        y = ref_configs.yaml_scalars(path)
        assert (c["w"], c["h"]) == (int(y["image_width"]), int(y["image_height"])), name
        assert (c["max_cnt"], c["min_dist"], c["max_iters"]) == (int(y["max_cnt"]), int(y["min_dist"]), int(y["max_num_iterations"])), name
        assert c["mask_morphology_size"] == (int(y["mask_morphology_size"]) if int(y["use_mask_morphology"]) else 0), name
        ov = c.get("overrides", ())          # keys an entry deliberately sets differently from the file it cites (zed_linepoint_dynamic: use_line)
        assert set(ov) <= {"use_line"}, name
        assert c["use_imu"] == int(y["imu"]) and ("use_line" in ov or c["use_line"] == int(y["use_line"])) and c["plane_constraint"] == int(y["plane_constraint"]), name
        assert c["keyframe_parallax"] == float(y["keyframe_parallax"]) and c["g_norm"] == float(y["g_norm"]), name
        assert c["noise"] == {k: float(y[k]) for k in ("acc_n", "gyr_n", "acc_w", "gyr_w")}, name
        assert (c["min_dynamic_dist"], c["max_dynamic_cnt"], c["instance_init_min_num"]) == (int(y["min_dynamic_dist"]), int(y["max_dynamic_cnt"]), int(y["instance_init_min_num"])), name
        assert c["use_det3d"] == int(y["use_det3d"]) and c["static_inst_threshold"] == float(y.get("static_inst_threshold", 10.0)), name
        assert c["every_second_frame"] == (y["dataset_type"].lower() != "kitti"), name
        if "cam0_calib" in y:
            for cam, key in ((c["cam0"], "cam0_calib"), (c["cam1"], "cam1_calib")):
                txt = open(os.path.join(os.path.dirname(path), y[key])).read().split()
                vals = {k.rstrip(":"): float(txt[i + 1]) for i, k in enumerate(txt) if k.rstrip(":") in ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2")}
                assert cam == vals, (name, key)


# ------------------------------------------------------------------- GPU: images -> trajectory at those parameter sets
INT_FIELDS = ["id", "is_initial", "is_tracking", "is_curr_visible", "is_static", "is_init_velocity", "age", "lost_number", "static_frame", "n_landmarks", "n_valid", "triangle_num"]


def run_config(oracle, name, frames, n_boxes=4):
    from dynamic_vins_amd import dynsim, sim
    from dynamic_vins_amd.backend import LINELM_DTYPE
    from dynamic_vins_amd.pipeline import DynamicPipeline, DynamicSequence
    from tests.conftest import iterations_agree
    from tests.test_dynamic_pipeline import rows_equal
    c = ref_configs.CONFIGS[name]
    w, h = c["w"], c["h"]
    traj = sim.Trajectory(z_amp=0.0) if c["plane_constraint"] else None
    seq = DynamicSequence(w, h, c["cam0"], frames, rate=20.0, boxes=("escort", n_boxes), baseline=c["baseline"], body_is_camera=c["body_is_camera"], cam1=c["cam1"], traj=traj)
    segs = sim.SegmentSim(seq.traj, c["cam0"], w, h, n=300, t_ic1=seq.rig["t_ic1"]) if c["use_line"] else None      # 1242x375 sees a narrow band of the room
    ekw = dict(ref_configs.est_kw(c), **c["noise"])
    pipe = DynamicPipeline(seq, max_cnt=c["max_cnt"], min_dist=c["min_dist"], max_iters=c["max_iters"], use_imu=c["use_imu"], max_dynamic_cnt=c["max_dynamic_cnt"],
                           min_dynamic_dist=c["min_dynamic_dist"], use_det3d=c["use_det3d"], static_inst_threshold=c["static_inst_threshold"],
                           mask_morphology_size=c["mask_morphology_size"], segments=segs, est_kw=ekw)
    cam0t, cam1t = sim.cam_tuple(c["cam0"]), sim.cam_tuple(c["cam1"])
    trk = oracle.tracker(w, h, c["max_cnt"], c["min_dist"], 1, 1, cam0t, cam1t)
    oin = oracle.insts(trk, c["max_dynamic_cnt"], c["min_dynamic_dist"], c["use_det3d"])
    est = oracle.estimator(**pipe.est_kw)
    k_imu = 0
    st = dict(obj_rows=0, objs=set(), initial=0, solved=0, max_dp=0.0, obj_p=0.0, obj_q=0.0, min_dets=10 ** 9, bg_rows=0, lines=0, line_tri=0, nonlinear=0, iter_mismatch=0)
    dev_p, ref_p = [], []
    for k in range(frames):
        t = seq.times[k]
        sd = pipe.step()
        while k_imu < len(seq.imu_t) and seq.imu_t[k_imu] <= t + 0.006:
            est.input_imu(seq.imu_t[k_imu], seq.imu_a[k_imu], seq.imu_g[k_imu]); k_imu += 1
        left, right = seq.host_frame(k)
        rows_o = trk.track_image(left, right, t, mask=seq.inv_mask[k], mode=2, erode_k=c["mask_morphology_size"])
        oin.set_disparity(seq.disp_host(k), seq.baseline)
        io, fo, po = oin.track(left, right, t, seq.dets[k], seq.boxes3d[k] if c["use_det3d"] else None, dynsim.INSTOBS_DTYPE, dynsim.BOX3D_DTYPE)
        rows_equal(pipe.rows, rows_o, f"{name} frame {k} background")
        assert len(io) == len(pipe.insts), f"frame {k}: {len(io)} vs {len(pipe.insts)} objects"
        for fld in ["id", "has_box3d", "first_feat", "n_feats", "first_point", "n_points"]:
            assert np.array_equal(io[fld], pipe.insts[fld]), f"frame {k}: {fld}"
        assert np.array_equal(io["rect"], pipe.insts["rect"]) and io["box3d"].tobytes() == pipe.insts["box3d"].tobytes(), f"frame {k}"
        rows_equal(pipe.ifeats, fo, f"{name} frame {k} objects")
        assert np.array_equal(po, pipe.ipts)
        st["obj_rows"] += len(fo); st["objs"].update(int(i) for i in io["id"]); st["min_dets"] = min(st["min_dets"], len(io)); st["bg_rows"] += len(rows_o)
        if segs is not None:
            # the line half of the hand-over: UndistortedLineEndPoints of the same pixel segments on both sides, bit for bit
            il, sl, ir, sr = pipe.seg_px
            un_l = oracle.lift_projective(cam0t, sl.reshape(-1, 2)).reshape(-1, 4).astype(np.float64)
            un_r = oracle.lift_projective(cam1t, sr.reshape(-1, 2)).reshape(-1, 4).astype(np.float64)
            lrows_o = sim.line_rows(il, un_l, ir, un_r)
            assert lrows_o.tobytes() == pipe.lrows.tobytes(), f"frame {k}: line rows"
            est.set_lines(lrows_o)
        rc, so = est.process_dynamic(rows_o, t, io, fo, po)
        assert rc == 0
        assert (sd.frame, sd.nonlinear, sd.margin_old, sd.n_landmarks, sd.n_long) == (so.frame, so.nonlinear, so.margin_old, so.n_landmarks, so.n_long), f"frame {k}"
        assert iterations_agree(sd, so), f"frame {k}: iterations {sd.iterations} vs {so.iterations}, costs {sd.initial_cost} vs {so.initial_cost}"
        st["iter_mismatch"] += int(sd.iterations != so.iterations)
        Wd, Wo = pipe.est.window(), est.window()
        st["max_dp"] = max(st["max_dp"], np.abs(Wd[:, :3] - Wo[:, :3]).max())
        if sd.nonlinear:
            st["nonlinear"] += 1
            dev_p.append(Wd[10, :3].copy()); ref_p.append(Wo[10, :3].copy())
        Io, So = est.instances(dynsim.INSTSTATE_DTYPE)
        Id, Sd = pipe.est.instances()
        assert len(Io) == len(Id)
        for fld in INT_FIELDS:
            assert np.array_equal(Io[fld], Id[fld]), f"frame {k}: {fld} {Io[fld]} vs {Id[fld]}"
        assert So[0] == Sd[0] and So[1] == Sd[1], f"frame {k}: {So} vs {Sd}"
        st["solved"] += int(So[0] > 0)
        for a, b in zip(Io, Id):
            st["initial"] += int(a["is_initial"])
            st["obj_p"] = max(st["obj_p"], np.abs(a["window"][:, :3] - b["window"][:, :3]).max())
            qa, qb = a["window"][:, 3:], b["window"][:, 3:]
            sg = np.sign((qa * qb).sum(1, keepdims=True)); sg[sg == 0] = 1
            st["obj_q"] = max(st["obj_q"], np.abs(qa - sg * qb).max())
        if segs is not None:
            Ld, Lo = pipe.est.lines(), est.lines(LINELM_DTYPE)
            assert len(Ld) == len(Lo)
            for fld in ("id", "start_frame", "n_obs", "is_triangulation"):
                assert np.array_equal(Ld[fld], Lo[fld]), f"frame {k}: line {fld}"
            st["lines"] = max(st["lines"], len(Lo)); st["line_tri"] = max(st["line_tri"], int(Lo["is_triangulation"].sum()))
    ate_gt = pipe.ate()
    pipe.ctx.close()
    ate_vs_oracle = sim.align_ate(np.array(dev_p), np.array(ref_p))[0] if len(dev_p) >= 3 else None
    st["dev_traj"] = np.array(dev_p)
    return st, ate_gt, ate_vs_oracle


def check(st, ate_vs_oracle, frames):
    assert st["min_dets"] >= 3, st                                      # objects in EVERY frame (north_star's "VIODE-dynamic", not an occasional visitor)
    assert st["obj_rows"] > 20 * frames and len(st["objs"]) >= 3 and st["initial"] > 10 and st["solved"] > 5, st
    assert st["nonlinear"] >= frames - 12
    from tests.test_dynamic_pipeline import bars
    b = bars(st)                                                        # strict unless a window solve ended one iteration apart (documented there)
    assert st["max_dp"] < b[0] and st["obj_p"] < max(b[1], 5e-5) and st["obj_q"] < max(b[2], 2e-5), st      # object orientation: 2e-5 rad (the object solve's box-orientation term
    assert st["iter_mismatch"] <= 2, st                                 # amplifies ego differences of 1e-7 by ~100 where the box fit is weak: the plane-constrained KITTI set shows 1.2e-5)
    assert ate_vs_oracle is not None and ate_vs_oracle < 1e-3, ate_vs_oracle      # north_star's bar (in practice ~1e-8)


@pytest.mark.gpu
def test_viode_yaml_parameters_dynamic_from_pixels(oracle):
    st, ate_gt, ate_o = run_config(oracle, "viode", 40)
    check(st, ate_o, 40)
    assert ate_gt < 0.1, ate_gt


@pytest.mark.gpu
def test_zed_dynamic_yaml_parameters_from_pixels(oracle):
    st, ate_gt, ate_o = run_config(oracle, "zed_dynamic", 36)
    check(st, ate_o, 36)
    assert st["bg_rows"] > 300 * 36, st                                  # max_cnt 400 is really reached, not capped at 250
    assert ate_gt < 0.1, ate_gt


@pytest.mark.gpu
def test_kitti_tracking_online_line_point_dynamic_from_pixels(oracle):
    st, ate_gt, ate_o = run_config(oracle, "kitti_tracking_online", 36)
    check(st, ate_o, 36)
    assert st["lines"] >= 10 and st["line_tri"] >= 3, st          # (36 frames of a 1242x375 view: few segments stay long enough to be triangulated)


@pytest.mark.gpu
def test_zed_1280x720_line_point_dynamic_from_pixels(oracle):
    """BASELINE.json config 5 as stated: ZED 1280x720, 400 features / min_dist 25, erosion 20, vision only, use_det3d 1 — LinePoint AND dynamic together.
    Same bars as the other parameter sets (background / object rows bit-identical, line tables identical on every frame, window and object states against the
    oracle) and, because the reference's lineProjectionFactor::sqrt_info is zero, the ego trajectory must equal the use_line 0 run of the same
    sequence up to ceres' parameter-tolerance norm (the line blocks only count in |x|)."""
    frames = 36
    st, ate_gt, ate_o = run_config(oracle, "zed_linepoint_dynamic", frames)
    check(st, ate_o, frames)
    assert st["bg_rows"] > 300 * frames, st
    assert st["lines"] >= 10 and st["line_tri"] >= 3, st
    assert ate_gt < 0.1, ate_gt
    st0, _, _ = run_config(oracle, "zed_dynamic", frames)
    a, b = st["dev_traj"], st0["dev_traj"]
    assert a.shape == b.shape and np.abs(a - b).max() < 1e-6, np.abs(a - b).max()
