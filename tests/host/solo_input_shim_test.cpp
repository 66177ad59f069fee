// The shim's detector-input classes (dvins_shim.hpp: dynamic_vins::Pipeline with image_info / ProcessInput / ProcessInputEnqueue / ProcessInputCollect, and
// Detector2D::ForwardTensor) compile against include/dvins.h with -Wall -Werror and link against the library.  "check": without a ctx the construction throws, by name.
// "run SCENE OUT": a scene written by tests/test_solo_input_shim.py (int32 width height model_w model_h n_frames channels n_classes grid fh fw; the kernel map, the
// category map and the mask feature as float32; per frame height x width x 3 bytes) — per frame Pipeline::ProcessInput's tensor is appended to OUT (ProcessInput, then
// Enqueue + Collect into the other buffer) and "k rect ..." is printed; then Detector2D::ForwardTensor with a stand-in network that returns the scene's outputs and
// Detector2D::ForwardHead on the same outputs print "tensor ..." and "head ..." with labels, scores and rectangles.
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <fstream>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

static std::string frame_line(bool any, const SoloSeg& s, InstsFeatManager& insts) {
    char buf[128];
    std::string out = any ? "1" : "0";
    for (int i = 0; i < s.n; ++i) { std::snprintf(buf, sizeof(buf), " %d:%a", s.cate_labels[i], (double)s.cate_scores[i]); out += buf; }
    if (any)
        for (const dv_inst_det& d : insts.StackFrameCollect(2).dets) { std::snprintf(buf, sizeof(buf), " [%d %d %d %d]", d.x, d.y, d.w, d.h); out += buf; }
    return out;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        try { Pipeline p(nullptr, 64, 32); } catch (const std::exception& ex) { std::printf("refused: %s\n", ex.what()); return 0; }
        return 1;
    }
    if (argc > 3 && !std::strcmp(argv[1], "run")) {
        using copy_fn = int (*)(void*, const void*, size_t, int);
        copy_fn copy = reinterpret_cast<copy_fn>(dlsym(RTLD_DEFAULT, "hipMemcpy"));      // the runtime the library has loaded: device -> host of the stage's tensor
        if (!copy) { std::printf("no hipMemcpy\n"); return 2; }
        std::ifstream f(argv[2], std::ios::binary);
        std::ofstream out(argv[3], std::ios::binary);
        int32_t hd[10];
        f.read((char*)hd, sizeof(hd));
        const int W = hd[0], H = hd[1], MW = hd[2], MH = hd[3], NF = hd[4], CH = hd[5], NC = hd[6], G = hd[7], FH = hd[8], FW = hd[9];
        std::vector<float> kern((size_t)CH * G * G), cate((size_t)NC * G * G), feat((size_t)CH * FH * FW);
        f.read((char*)kern.data(), kern.size() * 4); f.read((char*)cate.data(), cate.size() * 4); f.read((char*)feat.data(), feat.size() * 4);
        dv_config c{};
        c.width = W; c.height = H; c.max_cnt = 30; c.min_dist = 10; c.flow_back = 1; c.stereo = 1;
        c.cam0.fx = c.cam0.fy = 100; c.cam0.cx = W / 2; c.cam0.cy = H / 2; c.cam1 = c.cam0;
        {
            FeatureTracker tracker(c);
            InstsFeatManager insts(tracker, 50, 5, 0);
            Pipeline pipe(tracker.ctx(), MW, MH);
            std::vector<uint8_t> img((size_t)W * H * 3);
            std::vector<float> host((size_t)3 * MW * MH);
            ImageView view{img.data(), W, H, 3 * W, false, true};
            for (int k = 0; k < NF; ++k) {
                f.read((char*)img.data(), img.size());
                const float* a = pipe.ProcessInput(view);
                if (copy(host.data(), a, host.size() * 4, 2) != 0) return 4;
                out.write((const char*)host.data(), host.size() * 4);
                pipe.ProcessInputEnqueue(view);
                const float* b = pipe.ProcessInputCollect();
                if (copy(host.data(), b, host.size() * 4, 2) != 0) return 4;
                out.write((const char*)host.data(), host.size() * 4);
                const ImageInfo& i = pipe.image_info;
                std::printf("%d rect %d %d %d %d %d %d other %d\n", k, i.rect_x, i.rect_y, i.rect_w, i.rect_h, i.origin_w, i.origin_h, (int)(a != b));
            }
            dv_solo_outputs o{};
            o.n_levels = 1; o.channels = CH; o.n_classes = NC; o.mem = DV_MEM_HOST; o.kernel[0] = kern.data(); o.cate[0] = cate.data(); o.grid[0] = G; o.fh = FH; o.fw = FW; o.feature = feat.data();
            dv_solo_params p{};
            p.score_thr = 0.1f; p.mask_thr = 0.5f; p.update_thr = 0.05f; p.nms_sigma = 2.0f; p.nms_pre = 16; p.max_per_img = 16; p.nms_kernel = DV_SOLO_NMS_GAUSSIAN; p.max_candidates = 16;
            p.num_grids[0] = G; p.strides[0] = 8.0f;
            Detector2D det(tracker.ctx(), p, MW, MH, W, H);
            const float* seen = nullptr;
            SoloSeg sa, sb;
            const bool ta = det.ForwardTensor(view, [&](const float* input) { seen = input; return o; }, insts, &sa);
            std::printf("tensor %s\n", frame_line(ta, sa, insts).c_str());
            const bool tb = det.ForwardHead(o, insts, &sb);
            std::printf("head %s\n", frame_line(tb, sb, insts).c_str());
            if (!seen || copy(host.data(), seen, host.size() * 4, 2) != 0) return 4;
            out.write((const char*)host.data(), host.size() * 4);      // what the network was handed: the last frame's input once more
        }
        return 0;
    }
    return 3;
}
