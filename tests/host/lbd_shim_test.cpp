// The shim's LBD half (dvins_shim.hpp: LineDetector::Describe / DescribeEnqueue / DescribeCollect and FeatureTracker::TrackImageLine's overload for undescribed LSD
// output) compiles against include/dvins.h with -Wall -Werror and links against the library.  "check": the refusals that need no device.  "run FILE": a scenario written
// by tests/test_lbd_shim.py (int32 w, h, n_frames; per frame the left and the right image, w x h bytes each, int32 n_left, n_left x 6 float32, int32 n_right,
// n_right x 6 float32) through DescribeEnqueue on both cams, DescribeCollect (even frames with a host copy of the rows, odd frames without) and Track; prints per frame
// "k | dl src[:64 hex digits] ... | dr ... | left id:src:cnt ... | right id:src ... | rows id:has_right ...", src being indices into the LSD arrays.  "image FILE": the
// same scenario through TrackImageLine(img, left_keylines, right_keylines, first); prints per frame "k | kept nl nr | lines id:n_entries:x1:y1:x2:y2[...] ..." (doubles
// as %a) and fails if a descriptor row reached the host.
#include <cstdio>
#include <cstring>
#include <fstream>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

struct Frame { std::vector<uint8_t> left, right; std::vector<dv_key_line> kl, kr; };

static std::vector<Frame> read_scenario(const char* path, int* w, int* h) {
    std::ifstream f(path, std::ios::binary);
    int32_t hdr[3] = { 0, 0, 0 };
    f.read((char*)hdr, 12);
    *w = hdr[0]; *h = hdr[1];
    std::vector<Frame> frames((size_t)hdr[2]);
    for (Frame& fr : frames) {
        fr.left.resize((size_t)*w * *h); fr.right.resize((size_t)*w * *h);
        f.read((char*)fr.left.data(), (std::streamsize)fr.left.size()); f.read((char*)fr.right.data(), (std::streamsize)fr.right.size());
        int32_t n = 0;
        f.read((char*)&n, 4); fr.kl.resize((size_t)n); if (n) f.read((char*)fr.kl.data(), (std::streamsize)n * sizeof(dv_key_line));
        f.read((char*)&n, 4); fr.kr.resize((size_t)n); if (n) f.read((char*)fr.kr.data(), (std::streamsize)n * sizeof(dv_key_line));
    }
    return frames;
}

static dv_config config(int w, int h) {
    dv_config c{};
    c.width = w; c.height = h; c.max_cnt = 30; c.min_dist = 10; c.flow_back = 1; c.stereo = 1;
    c.cam0.fx = 460; c.cam0.fy = 458; c.cam0.cx = 367; c.cam0.cy = 248; c.cam0.k1 = -0.28; c.cam0.k2 = 0.07; c.cam1 = c.cam0;
    return c;
}

static void print_described(const char* tag, const FrameLines& f) {
    std::printf(" | %s", tag);
    for (size_t i = 0; i < f.keylsd.size(); ++i) {
        std::printf(" %d", f.src[i]);
        if (!f.lbd_descr.empty()) { std::printf(":"); for (uint8_t b : f.lbd_descr[i]) std::printf("%02x", b); }
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        int refused = 0;
        std::vector<uint8_t> px(96 * 40, 0);
        const ImageView gray{ px.data(), 96, 40, 96, false }, bgr{ px.data(), 32, 40, 96, false, true }, small{ px.data(), 48, 40, 48, false }, dev_mask{ px.data(), 96, 40, 96, true };
        std::vector<dv_key_line> lines(3, dv_key_line{ 3, 4, 30, 9, 0.18f, 27.5f });
        std::vector<int32_t> two(2, 28);
        LineDetector det(nullptr, true);          // every refusal below comes before the library is asked
        try { det.DescribeEnqueue(2, gray, lines); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { det.DescribeEnqueue(0, bgr, lines); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { det.DescribeEnqueue(0, ImageView{}, lines); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { det.DescribeEnqueue(0, gray, lines, &two); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { det.DescribeEnqueue(0, gray, lines, nullptr, &small); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { det.DescribeEnqueue(0, gray, lines, nullptr, &dev_mask); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { det.DescribeCollect(0); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        FrameLines on_dev, on_host;
        on_dev.device = true; on_host.keylsd.resize(2); on_host.lbd_descr.resize(2);
        try { LineDetector::Check(on_dev, &on_host); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { LineDetector::Check(on_dev); LineDetector::Check(on_dev, &on_dev); std::printf("accepted\n"); } catch (const std::exception& e) { std::printf("wrongly refused: %s\n", e.what()); return 1; }
        return refused == 8 ? 0 : 1;
    }
    if (argc > 2 && !std::strcmp(argv[1], "run")) {
        int w = 0, h = 0;
        const std::vector<Frame> frames = read_scenario(argv[2], &w, &h);
        const dv_config c = config(w, h);
        dv_ctx* ctx = dv_create(&c);
        if (!ctx) { std::printf("dv_create: %s\n", dv_last_error(nullptr)); return 2; }
        {
            LineDetector det(ctx, true);
            FrameLines::Ptr prev;
            for (size_t k = 0; k < frames.size(); ++k) {
                const Frame& fr = frames[k];
                det.DescribeEnqueue(0, ImageView{ fr.left.data(), w, h, w, false }, fr.kl);
                det.DescribeEnqueue(1, ImageView{ fr.right.data(), w, h, w, false }, fr.kr);
                FrameLines::Ptr left = det.DescribeCollect(0, k % 2 == 0), right = det.DescribeCollect(1, k % 2 == 0);
                if (!left->device || !left->dev_desc || (k % 2 && !left->lbd_descr.empty())) { std::printf("not a device frame\n"); return 4; }
                std::printf("%zu", k);
                print_described("dl", *left); print_described("dr", *right);
                if (k % 2) det.Track(prev, left, right);
                else { det.TrackLeftLine(prev, left); det.TrackRightLine(left, right); }
                if (left->device || left->dev_desc || left->keylsd.size() != left->line_ids.size() || left->src.size() != left->line_ids.size()) { std::printf("\nleft set not reordered\n"); return 4; }
                std::printf(" | left");
                for (size_t i = 0; i < left->line_ids.size(); ++i) {
                    const auto it = left->track_cnt.find(left->line_ids[i]);
                    std::printf(" %u:%d:%d", left->line_ids[i], left->src[i], it == left->track_cnt.end() ? 0 : it->second);
                    const dv_key_line &a = left->keylsd[i], &b = fr.kl.at((size_t)left->src[i]);
                    if (std::memcmp(&a, &b, sizeof a)) { std::printf("\nsrc does not name the LSD line\n"); return 4; }
                }
                std::printf(" | right");
                for (size_t i = 0; i < right->line_ids.size(); ++i) std::printf(" %u:%d", right->line_ids[i], right->src[i]);
                std::printf(" | rows");
                for (const dv_line_row& r : det.rows()) std::printf(" %u:%d", r.id, r.has_right);
                std::printf("\n");
                prev = left;
            }
        }
        dv_destroy(ctx);
        return 0;
    }
    if (argc > 2 && !std::strcmp(argv[1], "image")) {
        int w = 0, h = 0;
        const std::vector<Frame> frames = read_scenario(argv[2], &w, &h);
        FeatureTracker tracker(config(w, h));
        for (size_t k = 0; k < frames.size(); ++k) {
            const Frame& fr = frames[k];
            SemanticImage img;
            img.gray0 = ImageView{ fr.left.data(), w, h, w, false };
            img.gray1 = ImageView{ fr.right.data(), w, h, w, false };
            img.time0 = 1.0 + 0.05 * (double)k; img.seq = (unsigned)k;
            FrameLines::Ptr left, right;
            const FeatureBackground fb = tracker.TrackImageLine(img, fr.kl, fr.kr, k == 0, nullptr, nullptr, 60.0f, &left, &right);
            if (!left || !right || !left->lbd_descr.empty() || !right->lbd_descr.empty()) { std::printf("a descriptor row reached the host\n"); return 4; }
            std::printf("%zu | kept %zu %zu | lines", k, left->keylsd.size(), right->keylsd.size());
            for (const auto& kv : fb.lines) {
                std::printf(" %u:%zu", kv.first, kv.second.size());
                for (const auto& ob : kv.second) std::printf(":%a:%a:%a:%a", ob.second.x1, ob.second.y1, ob.second.x2, ob.second.y2);
            }
            std::printf("\n");
        }
        return 0;
    }
    return 3;
}
