// The shim's stereo matcher (dvins_shim.hpp: dynamic_vins::MyStereoMatcher with Launch / WaitResult, and InstsFeatManager::SetDisparity on its device map) compiles
// against include/dvins.h with -Wall -Werror and links against the library.  "check": without a ctx the construction throws, by name.  "run SCENE OUT": a scene written
// by tests/test_stereo_sgm_pipeline.py (int32 width height n_disp n_frames; per frame the left and the right gray image, height x width bytes each) — per frame
// WaitResult's map is appended to OUT; then "alternating A points P" is printed: A = consecutive maps lie in different buffers, P = InstsFeatManager took the last map.
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        try { MyStereoMatcher m(nullptr); } catch (const std::exception& ex) { std::printf("refused: %s\n", ex.what()); return 0; }
        return 1;
    }
    if (argc > 3 && !std::strcmp(argv[1], "run")) {
        using copy_fn = int (*)(void*, const void*, size_t, int);
        copy_fn copy = reinterpret_cast<copy_fn>(dlsym(RTLD_DEFAULT, "hipMemcpy"));      // the runtime the library has loaded: device -> host of the stage's map
        if (!copy) { std::printf("no hipMemcpy\n"); return 2; }
        std::ifstream f(argv[2], std::ios::binary);
        std::ofstream out(argv[3], std::ios::binary);
        int32_t hd[4];
        f.read((char*)hd, sizeof(hd));
        const int W = hd[0], H = hd[1], D = hd[2], NF = hd[3];
        dv_config c{};
        c.width = W; c.height = H; c.max_cnt = 30; c.min_dist = 10; c.flow_back = 1; c.stereo = 1;
        c.cam0.fx = c.cam0.fy = 100; c.cam0.cx = W / 2; c.cam0.cy = H / 2; c.cam1 = c.cam0;
        {
            FeatureTracker tracker(c);
            InstsFeatManager insts(tracker, 50, 5, 0);
            MyStereoMatcher matcher(tracker.ctx(), D);
            std::vector<uint8_t> l((size_t)W * H), r((size_t)W * H);
            std::vector<float> host((size_t)W * H);
            bool alternating = true, took = false;
            const float* prev = nullptr;
            for (int k = 0; k < NF; ++k) {
                f.read((char*)l.data(), l.size()); f.read((char*)r.data(), r.size());
                matcher.Launch(ImageView{l.data(), W, H, W, false, false}, ImageView{r.data(), W, H, W, false, false});
                const DisparityMap m = matcher.WaitResult();
                if (m.empty() || m.width != W || m.height != H || m.stride_bytes != 4 * W) return 5;
                if (copy(host.data(), m.data, host.size() * 4, 2) != 0) return 4;
                out.write((const char*)host.data(), host.size() * 4);
                if (prev && prev == m.data) alternating = false;
                prev = m.data;
                if (k == NF - 1) { insts.SetDisparity(m, 0.12); took = true; }
            }
            std::printf("alternating %d points %d\n", (int)alternating, (int)took);
        }
        return 0;
    }
    return 3;
}
