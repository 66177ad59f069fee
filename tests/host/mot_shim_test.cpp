// The shim's multi-object tracker (dvins_shim.hpp: dynamic_vins::DeepSORT with update / update_enqueue / update_collect and AddInstancesByTracking) compiles against
// include/dvins.h with -Wall -Werror and links against the library.  "check": the refusal of a bad parameter set, no device.  "run FILE": a scenario written by
// tests/test_mot_shim.py (int32 n_init max_age budget feat_dim max_tracks n_frames; per frame int32 n, n x 4 int32 rectangles, n x feat_dim float32 embeddings) through
// AddInstancesByTracking, the embeddings alternately in host and in pinned memory; prints per frame "k n_tracks n_confirmed plane:id ..." of the detections that stay.
#include <cstdio>
#include <cstring>
#include <fstream>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        dv_mot_params bad{3, 5, 0, 512, 128, {0, 0, 0}};
        try { DeepSORT t(nullptr, bad); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); return 0; }
        return 1;
    }
    if (argc > 2 && !std::strcmp(argv[1], "run")) {
        std::ifstream f(argv[2], std::ios::binary);
        int32_t hd[6];
        f.read((char*)hd, sizeof(hd));
        dv_config c{};
        c.width = 64; c.height = 48; c.max_cnt = 30; c.min_dist = 10; c.flow_back = 1; c.stereo = 1;
        c.cam0.fx = c.cam0.fy = 100; c.cam0.cx = 32; c.cam0.cy = 24; c.cam1 = c.cam0;
        dv_ctx* ctx = dv_create(&c);
        if (!ctx) { std::printf("dv_create: %s\n", dv_last_error(nullptr)); return 2; }
        {
            dv_mot_params p{hd[0], hd[1], hd[2], hd[3], hd[4], {0, 0, 0}};
            DeepSORT::Ptr mot = std::make_shared<DeepSORT>(ctx, p);
            float* pin = static_cast<float*>(dv_pinned_alloc((size_t)DV_STACK_MAX_PLANES * hd[3] * sizeof(float)));
            for (int k = 0; k < hd[5]; ++k) {
                int32_t n = 0;
                f.read((char*)&n, 4);
                std::vector<int32_t> r((size_t)n * 4); std::vector<float> e((size_t)n * hd[3]);
                f.read((char*)r.data(), r.size() * 4); f.read((char*)e.data(), e.size() * 4);
                std::vector<dv_inst_det> dets((size_t)n); std::vector<int32_t> planes((size_t)n);
                for (int j = 0; j < n; ++j) { dets[j] = dv_inst_det{}; dets[j].track_id = (uint32_t)j; dets[j].x = r[4 * j]; dets[j].y = r[4 * j + 1]; dets[j].w = r[4 * j + 2]; dets[j].h = r[4 * j + 3]; planes[j] = j; }
                if (k % 2) { std::memcpy(pin, e.data(), e.size() * 4); mot->AddInstancesByTracking(dets, planes, pin, DV_MEM_PINNED); }
                else mot->AddInstancesByTracking(dets, planes, e.data(), DV_MEM_HOST);
                std::printf("%d %d %d", k, mot->n_tracks(), mot->n_confirmed());
                for (size_t j = 0; j < dets.size(); ++j) std::printf(" %d:%u", planes[j], dets[j].track_id);
                std::printf("\n");
            }
            std::printf("tracks %zu\n", mot->tracks().size());
            mot->reset();
            std::printf("after reset %zu\n", mot->tracks().size());
            dv_pinned_free(pin);
        }
        dv_destroy(ctx);
        return 0;
    }
    return 3;
}
