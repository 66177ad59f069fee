// The estimator's window bookkeeping (csrc/est_window.h) as a stand-alone program for the sanitizers (tests/test_est_window_host.py, built by est.mk).
//   est_window_asan preint   reads sample streams from stdin, pushes them through Preint — two streams through the second-new merge of
//                            EstWindow::slide_window — and prints sum_dt, dp, dq (x y z w), dv, J[225], P[225] with %.17g, after the pushes and again after a repropagate
//   est_window_asan walk     a synthetic 16-frame stereo track through add_features (merge join and hash fallback), triangulate, pnp_frame, build_factors (into a buffer
//                            that overflows), the host reject_outliers and every branch of slide_window, with the invariants the header states checked after each frame.
//                            With IMU it also keeps the three per-slot sample buffers the estimator used to carry beside each Preint and checks that they never differ
//                            from the Preint's own.  Prints "est_window_host ok"; any failed check aborts.
#include <cstdio>
#include <cstdlib>
#include <set>
#include "est_window.h"

using namespace estw;

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); std::abort(); } } while (0)

static dv_est_config config(int use_imu) {
    dv_est_config c{};
    c.use_imu = use_imu; c.stereo = 1; c.max_iters = 8; c.keyframe_parallax = 10.0; c.init_depth = 5.0; c.g_norm = 9.81;
    c.acc_n = 0.1; c.gyr_n = 0.01; c.acc_w = 0.001; c.gyr_w = 0.0001;
    for (int k = 0; k < 2; ++k) c.ric[k][0] = c.ric[k][4] = c.ric[k][8] = 1.0;
    c.tic[1][0] = 0.1;
    return c;
}

// ---------------------------------------------------------------- preint ----
static double rd() { double v; CHECK(std::scanf("%lf", &v) == 1); return v; }
static d3 rd3() { const double x = rd(), y = rd(), z = rd(); return mk3(x, y, z); }
static void dump(const Preint& p) {
    std::printf("%.17g\n%.17g\n%.17g\n%.17g\n", p.sum_dt, p.dp.x, p.dp.y, p.dp.z);
    std::printf("%.17g\n%.17g\n%.17g\n%.17g\n%.17g\n%.17g\n%.17g\n", p.dq.x, p.dq.y, p.dq.z, p.dq.w, p.dv.x, p.dv.y, p.dv.z);
    for (int i = 0; i < 225; ++i) std::printf("%.17g\n", p.J[i]);
    for (int i = 0; i < 225; ++i) std::printf("%.17g\n", p.P[i]);
}
// stdin: acc0 gyr0 ba bg (3 each), noise (4), n, n x [dt acc gyr], m, m x [dt acc gyr] (the interval merged behind the first; m = 0: none), ba bg of the repropagate
static int preint_mode() {
    dv_est_config c = config(1);
    const d3 a0 = rd3(), g0 = rd3(), ba = rd3(), bg = rd3();
    c.acc_n = rd(); c.gyr_n = rd(); c.acc_w = rd(); c.gyr_w = rd();
    EstWindow E(c);
    E.frame = kWin; E.margin_old = false;
    E.acc_0 = a0; E.gyr_0 = g0; E.Bas[kWin - 1] = E.Bas[kWin] = ba; E.Bgs[kWin - 1] = E.Bgs[kWin] = bg;
    E.pre[kWin - 1] = E.new_preint(kWin - 1);
    d3 la = a0, lg = g0;
    const int n = (int)rd();
    for (int i = 0; i < n; ++i) { const double dt = rd(); la = rd3(); lg = rd3(); E.pre[kWin - 1]->push_back(dt, la, lg); }
    const int m = (int)rd();
    if (m > 0) {          // the next interval starts from the last sample, as process_imu leaves acc_0 / gyr_0; the second-new slide appends it
        E.acc_0 = la; E.gyr_0 = lg; E.pre[kWin] = E.new_preint(kWin);
        for (int i = 0; i < m; ++i) { const double dt = rd(); la = rd3(); lg = rd3(); E.pre[kWin]->push_back(dt, la, lg); }
        E.acc_0 = la; E.gyr_0 = lg;
        E.slide_window();
        CHECK(E.pre[kWin] && E.pre[kWin]->dts.empty() && (int)E.pre[kWin - 1]->dts.size() == n + m);
    }
    dump(*E.pre[kWin - 1]);
    const d3 rba = rd3(), rbg = rd3();
    E.pre[kWin - 1]->repropagate(rba, rbg);
    dump(*E.pre[kWin - 1]);
    return 0;
}

// ---------------------------------------------------------------- walk ----
struct Track { uint32_t id; d3 pw; int born, dies; };
struct Shadow {          // the per-slot sample buffers the estimator kept twice, maintained by the rules it used
    std::vector<double> dt[kWin + 1]; std::vector<d3> la[kWin + 1], av[kWin + 1];
    void push(int f, double t, d3 a, d3 g) { dt[f].push_back(t); la[f].push_back(a); av[f].push_back(g); }
    void clear_tail() { dt[kWin].clear(); la[kWin].clear(); av[kWin].clear(); }
    void slide(bool margin_old) {
        if (margin_old) { for (int i = 0; i < kWin; ++i) { dt[i].swap(dt[i + 1]); la[i].swap(la[i + 1]); av[i].swap(av[i + 1]); } }
        else for (size_t i = 0; i < dt[kWin].size(); ++i) push(kWin - 1, dt[kWin][i], la[kWin][i], av[kWin][i]);
        clear_tail();
    }
    void check(const EstWindow& E) const {
        for (int i = 0; i <= kWin; ++i) {
            if (!E.pre[i]) { CHECK(dt[i].empty()); continue; }
            const Preint& p = *E.pre[i];
            CHECK(p.dts == dt[i] && p.accs.size() == la[i].size() && p.gyrs.size() == av[i].size());
            for (size_t k = 0; k < la[i].size(); ++k) CHECK(!std::memcmp(&p.accs[k], &la[i][k], sizeof(d3)) && !std::memcmp(&p.gyrs[k], &av[i][k], sizeof(d3)));
        }
    }
};

static void check_window(const EstWindow& E, bool sorted) {
    std::set<int> ids;
    for (size_t i = 0; i < E.lms.size(); ++i) {
        const Lm& l = E.lms[i];
        CHECK(!l.obs.empty() && l.start >= 0 && l.end() <= E.frame);
        CHECK(ids.insert(l.id).second);                                   // one landmark per id on either path
        if (sorted && i) CHECK(E.lms[i - 1].id < l.id);
    }
}
static void check_tables(const EstWindow& E, bool staged) {
    CHECK((int)E.invd.size() == E.long_count() && E.lmt.size() == E.invd.size());
    CHECK(staged == (E.fac_out != nullptr));
    const dv_ba_factor* F = E.fac_out ? E.fac_out : E.fac.data();
    if (!E.fac_out) CHECK((int)E.fac.size() == E.nfac);
    std::vector<const Lm*> longs;
    for (auto& l : E.lms) if (l.obs.size() >= 4) longs.push_back(&l);
    int next = 0;
    for (size_t r = 0; r < E.lmt.size(); ++r) {
        const dv_ba_lm& t = E.lmt[r]; const Lm& l = *longs[r];
        CHECK(t.first == next && t.count > 0 && t.first + t.count <= E.nfac && t.anchor == l.start);
        int mask = 0; for (int j = l.start; j <= l.end(); ++j) mask |= 1 << j;
        CHECK(t.mask == mask);
        for (int k = t.first; k < t.first + t.count; ++k) {
            const dv_ba_factor& f = F[k];
            CHECK(f.lm == (int)r && f.lm < (int)E.lmt.size() && f.fi == t.anchor && f.fj >= f.fi && f.fj <= E.frame && f.kind >= 0 && f.kind <= 2 && (f.kind == 2) == (f.fi == f.fj));
        }
        next = t.first + t.count;
    }
    CHECK(next == E.nfac);
}

// constant-velocity body (0.1 m per frame along x, no rotation) in front of a cloud 4..8 m away; with IMU the samples say exactly that
static void walk(int use_imu, bool hostile_ids) {
    EstWindow E(config(use_imu));
    const double step = 0.1, frame_dt = 0.05;
    const d3 vel = mk3(step / frame_dt, 0, 0);
    if (use_imu) { E.Vs[0] = vel; E.init_pose = true; }
    std::vector<Track> tracks; uint32_t next_id = 100; unsigned rng = 12345u;
    auto rnd = [&]() { rng = rng * 1664525u + 1013904223u; return (rng >> 8) / 16777216.0; };
    auto spawn = [&](int f, uint32_t id) { tracks.push_back(Track{ id, mk3(-2.0 + 6.0 * rnd() + step * f, -1.0 + 2.0 * rnd(), 4.0 + 4.0 * rnd()), f, f + 3 + (int)(rnd() * 14) }); };
    for (int i = 0; i < 48; ++i) spawn(0, next_id++);
    std::vector<dv_ba_factor> staging(600);          // the early windows fit, the full ones (> 600 factors) fall back to the vector
    Shadow sh; int staged_seen = 0, vector_seen = 0, slides[2][2] = { { 0, 0 }, { 0, 0 } }, hash_frames = 0; size_t rejected = 0;
    for (int it = 0; it < 16; ++it) {
        const int fc = E.frame; const double t = frame_dt * it;
        if (use_imu) for (int k = 0; k < 5; ++k) { const double dt = frame_dt / 5; const d3 a = mk3(0, 0, E.cfg.g_norm), w = mk3(0, 0, 0); E.process_imu(dt, a, w); if (E.frame != 0) sh.push(E.frame, dt, a, w); }
        if (it > 0) for (int k = 0; k < 3; ++k) spawn(it, hostile_ids && it % 3 == 0 ? 1000 - next_id++ : next_id++);      // hostile: descending ids, and ascending ones below them afterwards
        std::vector<dv_feat> feats;
        const d3 body = mk3(step * it, 0, 0);
        for (auto& tr_ : tracks) {
            if (it < tr_.born || it > tr_.dies) continue;
            dv_feat f{}; f.id = tr_.id; f.has_right = (tr_.id % 5) != 0;
            const d3 pl = tr_.pw - body, pr = pl - mk3(0.1, 0, 0);
            f.left[0] = pl.x / pl.z; f.left[1] = pl.y / pl.z; f.left[2] = 1; f.right[0] = pr.x / pr.z; f.right[1] = pr.y / pr.z; f.right[2] = 1;
            // a gross outlier as a track's last observation (right image: the PnP seed does not read it): the host rejection has something to remove
            if (tr_.id % 7 == 0 && it == std::max(tr_.born + 4, 13)) { f.right[0] += 0.3; tr_.dies = it; }
            feats.push_back(f);
        }
        for (size_t i = 0; i + 1 < feats.size(); i += 2) std::swap(feats[i], feats[i + 1]);      // the caller's order is not the id order
        bool sorted_before = true; for (size_t i = 1; i < E.lms.size(); ++i) if (E.lms[i - 1].id >= E.lms[i].id) sorted_before = false;
        E.add_features(fc, feats.data(), (int)feats.size());
        E.headers[fc] = t;
        bool sorted_now = true; for (size_t i = 1; i < E.lms.size(); ++i) if (E.lms[i - 1].id >= E.lms[i].id) sorted_now = false;
        if (!hostile_ids) CHECK(sorted_before && sorted_now);
        if (!sorted_now) ++hash_frames;
        check_window(E, sorted_now);
        for (auto& tr_ : tracks) if (it >= tr_.born && it <= tr_.dies) {          // every feature of the frame landed in exactly its landmark, as the newest observation
            int hits = 0; for (auto& l : E.lms) if (l.id == (int)tr_.id) { ++hits; CHECK(l.end() == fc); }
            CHECK(hits == 1);
        }
        if (use_imu) { E.frame_pre.push_back(std::shared_ptr<Preint>(E.tmp_pre.release())); E.tmp_pre = E.new_preint(fc); }
        if (!use_imu || !E.nonlinear) E.pnp_frame(fc);
        E.triangulate();
        for (auto& l : E.lms) CHECK(l.depth > 0 || (l.obs.size() == 1 && !l.obs[0].stereo));
        // the PnP seed (float world points: 1e-7 relative) and the IMU propagation both find the pose the points were projected from
        if (fc > 0) CHECK(std::fabs(E.Ps[fc].x - body.x) < 1e-4 && std::fabs(E.Ps[fc].y) < 1e-4 && std::fabs(E.Ps[fc].z) < 1e-4);
        // the solve's tables and parameter blocks, there and back
        E.states_to_arrays();
        E.build_factors(false, staging.data(), (int)staging.size());
        const bool staged = E.nfac <= (int)staging.size();
        check_tables(E, staged);
        (staged ? staged_seen : vector_seen)++;
        E.arrays_to_states();
        for (auto& l : E.lms) if (l.obs.size() >= 4) CHECK(l.solve_flag == 1);
        if (E.nonlinear) { const size_t before = E.lms.size(); E.reject_outliers(nullptr); CHECK(E.lms.size() <= before); rejected += before - E.lms.size(); check_window(E, sorted_now); }
        if (fc == kWin) {          // six slides: second-new and old with nonlinear off (RemoveFront, RemoveBack), then with it on (RemoveFront, RemoveBackShiftDepth twice, RemoveFront)
            static const bool old_at[6] = { false, true, false, true, true, false };
            const int s = it - kWin;
            if (use_imu && s == 0) {          // InitEstimator's IMU alignment on a window that needs none: the PnP seeds' rotations (float points, ~1e-6 rad) over 0.05 s
                E.solve_gyro_bias();
                for (int j = 0; j <= kWin; ++j) { CHECK(norm(E.Bgs[j]) < 1e-3); E.pre[j]->repropagate(mk3(0, 0, 0), E.Bgs[j]); }
            }
            E.margin_old = old_at[s]; E.nonlinear = s >= 2;
            if (use_imu) sh.slide(E.margin_old);
            E.slide_window();
            slides[E.margin_old][E.nonlinear]++;
        } else {
            E.margin_old = true; E.slide_window();          // a window still filling: only the back-up of frame 0
            E.frame++; const int p = E.frame - 1; E.Ps[E.frame] = E.Ps[p]; E.Vs[E.frame] = E.Vs[p]; E.Rs[E.frame] = E.Rs[p]; E.Bas[E.frame] = E.Bas[p]; E.Bgs[E.frame] = E.Bgs[p];
        }
        check_window(E, sorted_now);
        if (use_imu) sh.check(E);
        E.update_latest_states();
    }
    CHECK(staged_seen > 0 && vector_seen > 0);
    CHECK(slides[0][0] == 1 && slides[1][0] == 1 && slides[0][1] == 2 && slides[1][1] == 2 && rejected > 0);
    CHECK(hostile_ids == (hash_frames > 0));
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "preint")) return preint_mode();
    if (argc == 2 && !std::strcmp(argv[1], "walk")) {
        walk(0, false); walk(0, true); walk(1, false);
        std::printf("est_window_host ok\n");
        return 0;
    }
    std::fprintf(stderr, "usage: est_window_asan preint|walk\n");
    return 2;
}
