// The shim's ReID extractor (dvins_shim.hpp: dynamic_vins::Extractor with load_form / extract, and DeepSORT's update(detections, ori_img) and image-taking
// AddInstancesByTracking) compiles against include/dvins.h with -Wall -Werror and links against the library.  "check FILE": load_form of a file of the wrong length is
// refused by name, no device.  "run WEIGHTS SCENE OUT": a scene written by tests/test_reid_shim.py (int32 width height n_frames n_init max_age; per frame int32 n,
// n x 4 int32 rectangles, height x width x 3 bytes) — per frame Extractor::extract's embeddings are appended to OUT, then DeepSORT::AddInstancesByTracking(dets,
// planes, image) runs on the same image and prints "k n_tracks n_confirmed plane:id ...".
#include <cstdio>
#include <cstring>
#include <fstream>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

int main(int argc, char** argv) {
    if (argc > 2 && !std::strcmp(argv[1], "check")) {
        Extractor e(nullptr);
        try { e.load_form(argv[2]); } catch (const std::exception& ex) { std::printf("refused: %s\n", ex.what()); return 0; }
        return 1;
    }
    if (argc > 4 && !std::strcmp(argv[1], "run")) {
        std::ifstream f(argv[3], std::ios::binary);
        std::ofstream out(argv[4], std::ios::binary);
        int32_t hd[5];
        f.read((char*)hd, sizeof(hd));
        dv_config c{};
        c.width = hd[0]; c.height = hd[1]; c.max_cnt = 30; c.min_dist = 10; c.flow_back = 1; c.stereo = 1;
        c.cam0.fx = c.cam0.fy = 100; c.cam0.cx = hd[0] / 2; c.cam0.cy = hd[1] / 2; c.cam1 = c.cam0;
        dv_ctx* ctx = dv_create(&c);
        if (!ctx) { std::printf("dv_create: %s\n", dv_last_error(nullptr)); return 2; }
        {
            Extractor::Ptr ext = std::make_shared<Extractor>(ctx);
            ext->load_form(argv[2]);
            dv_mot_params p{hd[3], hd[4], 100, DV_REID_FEAT_DIM, 128, {0, 0, 0}};
            DeepSORT mot(ctx, p);
            mot.set_extractor(ext);
            std::vector<uint8_t> img((size_t)hd[0] * hd[1] * 3);
            for (int k = 0; k < hd[2]; ++k) {
                int32_t n = 0;
                f.read((char*)&n, 4);
                std::vector<int32_t> r((size_t)n * 4);
                f.read((char*)r.data(), r.size() * 4);
                f.read((char*)img.data(), img.size());
                ImageView view{img.data(), hd[0], hd[1], 3 * hd[0], false, true};
                std::vector<std::array<float, 4>> rects((size_t)n);
                std::vector<dv_inst_det> dets((size_t)n); std::vector<int32_t> planes((size_t)n);
                for (int j = 0; j < n; ++j) {
                    rects[j] = {(float)r[4 * j], (float)r[4 * j + 1], (float)r[4 * j + 2], (float)r[4 * j + 3]};
                    dets[j] = dv_inst_det{}; dets[j].track_id = (uint32_t)j; dets[j].x = r[4 * j]; dets[j].y = r[4 * j + 1]; dets[j].w = r[4 * j + 2]; dets[j].h = r[4 * j + 3]; planes[j] = j;
                }
                const std::vector<float> e = ext->extract(view, rects);
                out.write((const char*)e.data(), e.size() * 4);
                mot.AddInstancesByTracking(dets, planes, view);
                std::printf("%d %d %d", k, mot.n_tracks(), mot.n_confirmed());
                for (size_t j = 0; j < dets.size(); ++j) std::printf(" %d:%u", planes[j], dets[j].track_id);
                std::printf("\n");
            }
            std::vector<std::array<float, 4>> none;
            std::printf("empty %zu %zu\n", ext->extract(ImageView{}, none).size(), mot.update(none, ImageView{}).size());
        }
        dv_destroy(ctx);
        return 0;
    }
    return 3;
}
