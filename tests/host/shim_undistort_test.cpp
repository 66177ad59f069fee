// The header shim with undistort_input: 1 (tests/test_host_shim_undistort.py).
//   parse <config>                          Config::Camera(0 / 1) (host only: dv_optimal_new_camera)
//   track <config> <frames.raw> <w> <h>     a FeatureTracker built from the file: the intrinsics it and an Estimator built from the same file report, then the
//                                           rows of the first (distorted) frame
//   mask  <config> <frames.raw> <w> <h>     the same frame through TrackImageNaive with an inverse instance mask (a rectangle of object pixels): the shim remaps it
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

static void print_cam(const char* tag, const dv_cam& c) {
    std::printf("%s %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", tag, c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2);
}

int main(int argc, char** argv) {
    try {
        if (argc < 3) return 2;
        const std::string mode = argv[1], cfg_path = argv[2];
        if (mode == "parse") {
            const Config c = ReadConfig(cfg_path);
            std::printf("undistort_input %d\n", c.undistort_input);
            print_cam("file0", c.front.cam0); print_cam("file1", c.front.cam1);
            print_cam("cam0", c.Camera(0)); print_cam("cam1", c.Camera(1));
            return 0;
        }
        if ((mode == "track" || mode == "mask") && argc >= 6) {
            const int w = std::atoi(argv[4]), h = std::atoi(argv[5]);
            std::vector<uint8_t> l((size_t)w * h), r((size_t)w * h);
            std::ifstream f(argv[3], std::ios::binary);
            f.read((char*)l.data(), (std::streamsize)l.size()); f.read((char*)r.data(), (std::streamsize)r.size());
            if (!f) { std::printf("short frame file\n"); return 1; }
            FeatureTracker trk(cfg_path);
            Estimator est(cfg_path);
            print_cam("tracker0", trk.cam0()); print_cam("tracker1", trk.cam1());
            print_cam("estimator0", est.cam0()); print_cam("estimator1", est.cam1());
            SemanticImage img;
            std::vector<uint8_t> inv((size_t)w * h, 255);
            if (mode == "mask") {
                for (int y = h / 4; y < h / 2; ++y) for (int x = w / 3; x < 2 * w / 3; ++x) inv[(size_t)y * w + x] = 0;
                img.inv_merge_mask = ImageView{ inv.data(), w, h, w, false, false };
            }
            img.gray0 = ImageView{ l.data(), w, h, w, false, false }; img.gray1 = ImageView{ r.data(), w, h, w, false, false }; img.time0 = 1.0;
            if (mode == "mask") trk.TrackImageNaive(img); else trk.TrackImage(img);
            std::printf("rows %d\n", trk.n_rows());
            for (int i = 0; i < trk.n_rows(); ++i) {
                const dv_feat& q = trk.rows()[i];
                std::printf("row %u %d %d", q.id, q.track_cnt, q.has_right);
                for (int k = 0; k < 7; ++k) std::printf(" %.17g", q.left[k]);
                for (int k = 0; k < 7; ++k) std::printf(" %.17g", q.has_right ? q.right[k] : 0.0);
                std::printf("\n");
            }
            return 0;
        }
        return 2;
    } catch (const std::exception& e) {
        std::printf("THROWN %s\n", e.what());
        return 1;
    }
}
