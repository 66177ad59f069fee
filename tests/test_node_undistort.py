"""dvins_node with undistort_input: 1 (cfg::is_undistort_input, utils/camera_model.cpp:479-504): a small sequence rendered through a camera with EuRoC's distortion and
written to disk goes through the node, which builds the new camera matrices and the maps on the device itself (dv_undistort_setup).  The trajectory file must equal the
Python pipeline's (Pipeline(undistort_input=True)) byte for byte, as the node's other modes are tested (tests/test_node.py); with `--undistort 0` it must not."""
import os
import subprocess

import pytest

from tests.test_node import CAM, CFG, NODE, write_pgm, write_png

@pytest.mark.gpu
def test_node_undistort_input_equals_the_python_pipeline(tmp_path):
    from dynamic_vins_amd import io_formats, sim
    from dynamic_vins_amd.pipeline import Pipeline, SyntheticSequence
    assert os.path.exists(NODE), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    w, h, frames = 320, 240, 36
    cam = sim.scaled_cam(sim.EUROC, w, h, 752, 480)
    seq = SyntheticSequence(w, h, cam, frames, rate=20.0, t0=0.0)
    sd = tmp_path / "MH_01"
    (sd / "left").mkdir(parents=True); (sd / "right").mkdir()
    for k in range(frames):
        l, r = seq.host_frame(k)
        write_pgm(sd / "left" / f"{k:06d}.pgm", l); write_png(sd / "right" / f"{k:06d}.png", r)
    with open(sd / "imu.csv", "w") as f:
        f.write("#timestamp [ns],w_RS_S_x [rad s^-1],w_RS_S_y,w_RS_S_z,a_RS_S_x [m s^-2],a_RS_S_y,a_RS_S_z\n")
        for t, a, g in zip(seq.imu_t, seq.imu_a, seq.imu_g):
            f.write("%.17g,%.17g,%.17g,%.17g,%.17g,%.17g,%.17g\n" % (t, g[0], g[1], g[2], a[0], a[1], a[2]))
    open(sd / "times.txt", "w").write("".join("%.17g\n" % t for t in seq.times))
    (tmp_path / "cfg").mkdir()
    cfg = str(tmp_path / "cfg" / "node.yaml")
    text = CFG.format(w=w, h=h).replace("undistort_input: 0", "undistort_input: 1").replace("max_cnt: 150", "max_cnt: 100").replace("min_dist: 20", "min_dist: 15")
    assert "undistort_input: 1" in text and "max_cnt: 100" in text and "min_dist: 15" in text
    open(cfg, "w").write(text)
    open(tmp_path / "cfg" / "cam.yaml", "w").write(CAM.format(w=w, h=h, **cam))
    name = "MH_01_VIO_raw_PointOnly_Odometry.txt"

    out = subprocess.run([NODE, cfg, str(sd), str(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "undistort_input" in out.stderr
    got = open(tmp_path / name).read().splitlines()

    pipe = Pipeline(seq, max_cnt=100, min_dist=15, max_iters=8, host_frames=True, ba_stride=2, est_kw=dict(keyframe_parallax=10.0, g_norm=9.81), undistort_input=True)
    want = []
    for k in range(frames):
        pipe.step()
        if k % 2 == 0:
            want.append(io_formats.trajectory_line(seq.times[k], pipe.est.window()[10, :7]))
    pipe.ctx.close()
    assert len(got) == len(want) == frames // 2
    assert got == want, [i for i, (a, b) in enumerate(zip(got, want)) if a != b][:5]
    assert sum(1 for ln in got if not ln.endswith("0.000000 0.000000 0.000000 0.000000 0.000000 0.000000 1.000000")) >= 4      # part of it is solved, not the identity

    # the override: the same file without the set-up tracks the distorted frames with the distorted camera — another trajectory
    (tmp_path / "off").mkdir()
    out = subprocess.run([NODE, cfg, str(sd), str(tmp_path / "off"), "--undistort", "0"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "undistort_input" not in out.stderr
    off = open(tmp_path / "off" / name).read().splitlines()
    assert len(off) == len(got) and off != got
    # and the other way round: a file that says 0, switched on from the command line
    open(cfg, "w").write(text.replace("undistort_input: 1", "undistort_input: 0"))
    (tmp_path / "on").mkdir()
    out = subprocess.run([NODE, cfg, str(sd), str(tmp_path / "on"), "--undistort", "1"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert open(tmp_path / "on" / name).read().splitlines() == got


def test_node_refuses_undistort_input_with_viode_masks(tmp_path):
    """masks and key images cut from the distorted segmentation images would not lie on the undistorted frames: the node refuses the combination (before it touches a
    device or an image) instead of tracking with misaligned masks; without the switch the same file is accepted up to the missing images"""
    assert os.path.exists(NODE), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    w, h = 64, 48
    text = CFG.format(w=w, h=h).replace('dataset_type: "custom"', 'dataset_type: "viode"').replace('slam_type: "raw"', 'slam_type: "naive"')
    text += 'rgb_to_label_file: "rgb_ids.txt"\ndynamic_label_id: [7]\n'
    open(tmp_path / "node.yaml", "w").write(text)
    open(tmp_path / "cam.yaml", "w").write(CAM.format(w=w, h=h, fx=40.0, fy=40.0, cx=32.0, cy=24.0, k1=-0.2, k2=0.03, p1=0.0, p2=0.0))
    open(tmp_path / "rgb_ids.txt", "w").write("id,r,g,b\n7,10,20,30\n3,1,2,3\n")
    (tmp_path / "seq").mkdir()
    r = subprocess.run([NODE, str(tmp_path / "node.yaml"), str(tmp_path / "seq"), str(tmp_path), "--undistort", "1"], capture_output=True, text=True)
    assert r.returncode != 0 and "undistort_input with VIODE segmentation masks is not supported" in r.stdout + r.stderr, r.stdout + r.stderr
    r = subprocess.run([NODE, str(tmp_path / "node.yaml"), str(tmp_path / "seq"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode != 0 and "not supported" not in r.stdout + r.stderr and "seq/left" in r.stdout + r.stderr, r.stdout + r.stderr
