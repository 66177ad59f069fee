// The shim's line tracker (dvins_shim.hpp: dynamic_vins::LineDetector over FrameLines, and FeatureTracker::TrackImageLine's overload for unmatched detections) compiles
// against include/dvins.h with -Wall -Werror and links against the library.  "check": the refusals of bad frames, no device.  "run FILE": a scenario written by
// tests/test_line_shim.py (int32 n_frames; per frame int32 n_left, n_left x 6 float32, n_left x 32 bytes, int32 n_right (-1: no right image), n_right x 6 float32,
// n_right x 32 bytes) through TrackLeftLine / TrackRightLine (odd frames: Track); prints per frame
// "k | left id:src:cnt ... | right id:src ... | rows id:has_right ...", the counts being FrameLines::track_cnt's entries (0 = none).  "image FILE": the same scenario
// through FeatureTracker::TrackImageLine's overload for unmatched detections over blank images; prints per frame "k | lines id:n_entries:x1:y1:x2:y2[:x1:y1:x2:y2] ..."
// from FeatureBackground::lines (doubles as %a), then, once, a frame whose image is refused: the enqueued lines must be collected on the way out ("recovered").
#include <cstdio>
#include <cstring>
#include <fstream>
#include "dvins_shim.hpp"

using namespace dynamic_vins;

static FrameLines::Ptr read_lines(std::ifstream& f, int n) {
    auto fl = std::make_shared<FrameLines>();
    fl->keylsd.resize((size_t)n); fl->lbd_descr.resize((size_t)n);
    if (n > 0) { f.read((char*)fl->keylsd.data(), (std::streamsize)n * sizeof(dv_key_line)); f.read((char*)fl->lbd_descr.data(), (std::streamsize)n * DV_LINE_DESC_BYTES); }
    return fl;
}

int main(int argc, char** argv) {
    if (argc > 1 && !std::strcmp(argv[1], "check")) {
        int refused = 0;
        FrameLines big; big.keylsd.resize(DV_LINE_MAX + 1); big.lbd_descr.resize(DV_LINE_MAX + 1);
        try { LineDetector::Check(big); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        FrameLines ok; ok.keylsd.resize(3); ok.lbd_descr.resize(3);
        try { LineDetector::Check(ok, &big); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        FrameLines odd; odd.keylsd.resize(3); odd.lbd_descr.resize(2);
        try { LineDetector::Check(odd); } catch (const std::exception& e) { std::printf("refused: %s\n", e.what()); ++refused; }
        try { LineDetector::Check(ok); LineDetector::Check(ok, &ok); FrameLines none; LineDetector::Check(none); std::printf("accepted\n"); } catch (const std::exception& e) { std::printf("wrongly refused: %s\n", e.what()); return 1; }
        return refused == 3 ? 0 : 1;
    }
    if (argc > 2 && !std::strcmp(argv[1], "run")) {
        std::ifstream f(argv[2], std::ios::binary);
        int32_t nf = 0;
        f.read((char*)&nf, 4);
        dv_config c{};
        c.width = 752; c.height = 480; c.max_cnt = 30; c.min_dist = 10; c.flow_back = 1; c.stereo = 1;
        c.cam0.fx = 460; c.cam0.fy = 458; c.cam0.cx = 367; c.cam0.cy = 248; c.cam0.k1 = -0.28; c.cam0.k2 = 0.07; c.cam1 = c.cam0;
        dv_ctx* ctx = dv_create(&c);
        if (!ctx) { std::printf("dv_create: %s\n", dv_last_error(nullptr)); return 2; }
        {
            LineDetector det(ctx, true);
            FrameLines::Ptr prev;
            for (int k = 0; k < nf; ++k) {
                int32_t nl = 0, nr = 0;
                f.read((char*)&nl, 4);
                FrameLines::Ptr left = read_lines(f, nl);
                f.read((char*)&nr, 4);
                FrameLines::Ptr right = nr >= 0 ? read_lines(f, nr) : nullptr;
                if (!right) det.Track(prev, left, nullptr);
                else if (k % 2) det.Track(prev, left, right);
                else { det.TrackLeftLine(prev, left); det.TrackRightLine(left, right); }
                std::printf("%d | left", k);
                for (size_t i = 0; i < left->line_ids.size(); ++i) {
                    const auto it = left->track_cnt.find(left->line_ids[i]);
                    std::printf(" %u:%d:%d", left->line_ids[i], left->src[i], it == left->track_cnt.end() ? 0 : it->second);
                }
                std::printf(" | right");
                if (right) for (size_t i = 0; i < right->line_ids.size(); ++i) std::printf(" %u:%d", right->line_ids[i], right->src[i]);
                std::printf(" | rows");
                for (const dv_line_row& r : det.rows()) std::printf(" %u:%d", r.id, r.has_right);
                std::printf("\n");
                if (left->keylsd.size() != left->line_ids.size() || left->lbd_descr.size() != left->line_ids.size()) { std::printf("left set not reordered\n"); return 4; }
                prev = left;
            }
        }
        dv_destroy(ctx);
        return 0;
    }
    if (argc > 2 && !std::strcmp(argv[1], "image")) {
        std::ifstream f(argv[2], std::ios::binary);
        int32_t nf = 0;
        f.read((char*)&nf, 4);
        dv_config c{};
        c.width = 752; c.height = 480; c.max_cnt = 30; c.min_dist = 10; c.flow_back = 1; c.stereo = 1;
        c.cam0.fx = 460; c.cam0.fy = 458; c.cam0.cx = 367; c.cam0.cy = 248; c.cam0.k1 = -0.28; c.cam0.k2 = 0.07; c.cam1 = c.cam0;
        std::vector<uint8_t> blank((size_t)c.width * c.height, 0);
        FeatureTracker tracker(c);
        FrameLines::Ptr left, right;
        for (int k = 0; k < nf; ++k) {
            int32_t nl = 0, nr = 0;
            f.read((char*)&nl, 4);
            left = read_lines(f, nl);
            f.read((char*)&nr, 4);
            right = nr >= 0 ? read_lines(f, nr) : nullptr;
            SemanticImage img;
            img.gray0 = ImageView{blank.data(), c.width, c.height, c.width, false};
            img.gray1 = img.gray0;
            img.time0 = 1.0 + 0.05 * k; img.seq = k;
            const FeatureBackground fb = tracker.TrackImageLine(img, left, right, k == 0);
            std::printf("%d | lines", k);
            for (const auto& kv : fb.lines) {
                std::printf(" %u:%zu", kv.first, kv.second.size());
                for (const auto& ob : kv.second) std::printf(":%a:%a:%a:%a", ob.second.x1, ob.second.y1, ob.second.x2, ob.second.y2);
                if (kv.second.empty() || kv.second[0].first != 0 || (kv.second.size() == 2 && kv.second[1].first != 1) || kv.second.size() > 2) { std::printf("\nbad entry\n"); return 4; }
            }
            std::printf("\n");
        }
        SemanticImage bad;
        bad.gray0 = ImageView{blank.data(), c.width / 2, c.height, c.width / 2, false};
        bad.gray1 = bad.gray0;
        bad.time0 = 1.0 + 0.05 * nf; bad.seq = nf;
        bool threw = false;
        try { tracker.TrackImageLine(bad, left, right); } catch (const std::exception&) { threw = true; }
        SemanticImage img;
        img.gray0 = ImageView{blank.data(), c.width, c.height, c.width, false};
        img.gray1 = img.gray0;
        img.time0 = 1.0 + 0.05 * (nf + 1); img.seq = nf + 1;
        tracker.TrackImageLine(img, left, right);      // would be refused ("previous frame not collected") had the refused frame's lines stayed in flight
        std::printf("%s\n", threw ? "recovered" : "the half-size image was not refused");
        return threw ? 0 : 5;
    }
    return 3;
}
