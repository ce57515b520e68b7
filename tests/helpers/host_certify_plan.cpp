// Host program over csrc/certify_plan.h for tests/test_certify_plan_host.py
// (g++ -std=c++17 -O1 -g -fsanitize=address,undefined; run as a child process, never loaded into python).
//   names                                  the counter enum's names in order, then the status constants
//   geometry                               every cluster span at every start position of every axis: "cases N", a "FAIL ..." line per violation
//   walk SEED                              the serial crop walk on random clustered candidate sets: "sets N crops M", "FAIL ..." lines
//   sizing H W MAX_BATCH N_OUT CROP MAXC [LIST CH NO_SMALL NO_CONE]     cert_sizing's answer as key=value
#include "../../upliftingtabletennis_amd/csrc/certify_plan.h"
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <set>
#include <vector>

using namespace ttup;

static const int EXTENTS[] = {168, 176, 352, 640, 704, 1280};
static const int SIDES[] = {160, 168, 176, 200};
static const int R = CERT_R;

static int small_of(int c) { return c >= 2 * R + 24 ? CERT_SMALL : 0; }          // as cert_sizing (where the crop is square and interior)

// one axis: the cluster [lo, hi] in a crop of class `small`
static long long check_axis(int full, int c, int lo, int hi, int small) {
    const int o = cert_crop_origin((lo + hi) / 2, c, full, R, small);
    int clo, chi;
    cert_core_range(o, c, full, R, small, clo, chi);
    long long bad = 0;
    if (o % 8 != 0 || o < 0 || o > full - c) { printf("FAIL origin full=%d c=%d lo=%d hi=%d small=%d o=%d\n", full, c, lo, hi, small, o); ++bad; }
    if (lo < clo || hi >= chi) { printf("FAIL cover full=%d c=%d lo=%d hi=%d small=%d o=%d core=[%d,%d)\n", full, c, lo, hi, small, o, clo, chi); ++bad; }
    // the core keeps R + 1 positions from a crop edge that is not an image edge (its 3x3 windows then keep R)
    if ((o != 0 && clo < o + R + 1) || (o + c != full && chi > o + c - R - 1) || (o == 0 && clo != 0) || (o + c == full && chi != full) || clo >= chi) {
        printf("FAIL core full=%d c=%d small=%d o=%d core=[%d,%d)\n", full, c, small, o, clo, chi); ++bad;
    }
    return bad;
}

static int geometry() {
    long long cases = 0, bad = 0;
    for (int full : EXTENTS)
        for (int side : SIDES) {
            const int c = side < full ? side : full;
            if ((full - c) % 8) { printf("FAIL extent %d side %d is not a valid pair\n", full, side); ++bad; continue; }
            const int max_span = c - 2 * R - 10 > 0 ? c - 2 * R - 10 : 0;          // the walk: span < c - 2 R - 9 (a lone candidate: 0)
            for (int span = 0; span <= max_span; ++span)
                for (int lo = 0; lo + span < full; ++lo) {
                    ++cases;
                    bad += check_axis(full, c, lo, lo + span, 0);
                    if (small_of(c) && span <= small_of(c) - 8) { ++cases; bad += check_axis(full, c, lo, lo + span, small_of(c)); }
                }
        }
    printf("cases %lld\nfailures %lld\n", cases, bad);
    return 0;
}

static uint64_t g_rng;
static unsigned rnd(unsigned n) {          // [0, n): splitmix64
    uint64_t z = (g_rng += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return (unsigned)(((z ^ (z >> 31)) >> 11) % n);
}

struct Crop { int y0, x0, small; };
static bool in_core(const Crop& k, int y, int x, int H, int W, int Hc, int Wc) {
    int ylo, yhi, xlo, xhi;
    cert_core_range(k.y0, Hc, H, R, k.small, ylo, yhi);
    cert_core_range(k.x0, Wc, W, R, k.small, xlo, xhi);
    return y >= ylo && y < yhi && x >= xlo && x < xhi;
}

// the plan kernel's decisions as a serial walk, without its budgets: a candidate goes to the first crop whose core holds it, the first
// candidate (index order) that none holds opens a new crop
static long long walk_set(const std::vector<int>& sorted, int H, int W, int side, long long* n_crops) {
    const int cnt = (int)sorted.size(), Hc = side < H ? side : H, Wc = side < W ? side : W;
    const int small = (Hc == Wc && Hc < H && Wc < W) ? small_of(Hc) : 0;
    std::vector<int> found(cnt, -1);
    std::vector<Crop> crops;
    long long bad = 0;
    size_t tried = 0;
    while (true) {
        for (; tried < crops.size(); ++tried)
            for (int i = 0; i < cnt; ++i)
                if (found[i] < 0 && in_core(crops[tried], sorted[i] / W, sorted[i] % W, H, W, Hc, Wc)) found[i] = (int)tried;
        int first = -1;
        for (int i = 0; i < cnt && first < 0; ++i) if (found[i] < 0) first = i;
        if (first < 0) break;
        if ((int)crops.size() >= cnt) { printf("FAIL walk: more than cnt=%d crops (H=%d W=%d side=%d)\n", cnt, H, W, side); return bad + 1; }
        const NewCrop n = cert_open_crop(sorted.data(), cnt, first, H, W, Hc, Wc, R, small);
        const Crop k{n.y0, n.x0, n.small};
        if (n.y0 % 8 || n.x0 % 8 || n.y0 < 0 || n.x0 < 0 || n.y0 > H - Hc || n.x0 > W - Wc || (n.small != 0 && n.small != small)) {
            printf("FAIL walk: crop (%d,%d,%d) H=%d W=%d side=%d\n", n.y0, n.x0, n.small, H, W, side); ++bad;
        }
        if (!in_core(k, sorted[first] / W, sorted[first] % W, H, W, Hc, Wc)) {
            printf("FAIL walk: crop (%d,%d,%d) does not cover its candidate %d (H=%d W=%d side=%d)\n", n.y0, n.x0, n.small, sorted[first], H, W, side);
            return bad + 1;          // (the walk would not end)
        }
        crops.push_back(k);
    }
    for (int i = 0; i < cnt; ++i) {
        const Crop& k = crops[found[i]];
        const int y = sorted[i] / W, x = sorted[i] % W;
        for (int t = 0; t < 9; ++t) {
            const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;          // zero padding outside the image, not read from the crop
            if (yy < k.y0 || yy >= k.y0 + Hc || xx < k.x0 || xx >= k.x0 + Wc) {
                printf("FAIL walk: (%d,%d) of candidate %d outside its crop (%d,%d) H=%d W=%d side=%d\n", yy, xx, sorted[i], k.y0, k.x0, H, W, side); ++bad;
            }
        }
    }
    *n_crops += (long long)crops.size();
    return bad;
}

static int walk(uint64_t seed) {
    g_rng = seed;
    const int frames[2][2] = {{352, 640}, {704, 1280}}, sides[2] = {160, 168}, BOX = 40;
    long long sets = 0, n_crops = 0, bad = 0;
    for (const auto& f : frames)
        for (int side : sides)
            for (int place = 0; place < 9; ++place)          // where the FIRST box lies: 0 anywhere, 1-4 the corners, 5-8 the edges
                for (int trial = 0; trial < 24; ++trial) {
                    const int H = f[0], W = f[1];
                    const int target = trial == 0 ? 1 : (trial == 1 ? 512 : 1 + (int)rnd(512));
                    const int n_clusters = 1 + (int)rnd(4);
                    std::set<int> idx;
                    for (int k = 0; k < n_clusters; ++k) {
                        int by = (int)rnd(H - BOX + 1), bx = (int)rnd(W - BOX + 1);
                        if (k == 0) {
                            if (place == 1 || place == 2 || place == 5) by = 0;
                            if (place == 3 || place == 4 || place == 6) by = H - BOX;
                            if (place == 1 || place == 3 || place == 7) bx = 0;
                            if (place == 2 || place == 4 || place == 8) bx = W - BOX;
                        }
                        const int share = (target + n_clusters - 1) / n_clusters;
                        const int want = share < BOX * BOX ? share : BOX * BOX;
                        // the box's own corners first, so that a box on an image edge has candidates ON that edge
                        const int corner[4][2] = {{0, 0}, {0, BOX - 1}, {BOX - 1, 0}, {BOX - 1, BOX - 1}};
                        size_t before = idx.size();
                        for (int q = 0; q < 4 && (int)(idx.size() - before) < want && idx.size() < 512; ++q) idx.insert((by + corner[q][0]) * W + bx + corner[q][1]);
                        for (int tries = 0; (int)(idx.size() - before) < want && idx.size() < 512 && tries < 20000; ++tries)
                            idx.insert((by + (int)rnd(BOX)) * W + bx + (int)rnd(BOX));
                    }
                    const std::vector<int> sorted(idx.begin(), idx.end());
                    if (sorted.empty() || sorted.size() > 512) { printf("FAIL generator: %zu candidates\n", sorted.size()); ++bad; continue; }
                    ++sets;
                    bad += walk_set(sorted, H, W, side, &n_crops);
                }
    printf("sets %lld crops %lld\nfailures %lld\n", sets, n_crops, bad);
    return 0;
}

int main(int argc, char** argv) {
    const char* cmd = argc > 1 ? argv[1] : "";
    if (!strcmp(cmd, "names") && argc == 2) {
        for (int k = 0; k < CERT_N_STATS; ++k) printf("stat %s\n", cert_stat_name(k));
        printf("status single=%d resolved=%d not_certified=%d guard=%d status_mask=%d flags_mask=%d pending=%d audit_only=%d\n", CERT_SINGLE, CERT_RESOLVED,
               CERT_NOT_CERTIFIED, CERT_GUARD, CERT_STATUS_MASK, CERT_FLAGS_MASK, CERT_PENDING, CERT_AUDIT_ONLY);
        printf("const max_k=%d max_frame_crops=%d r=%d small=%d sizeof_croprec=%zu\n", CERT_MAX_K, CERT_MAX_FRAME_CROPS, CERT_R, CERT_SMALL, sizeof(CropRec));
        return 0;
    }
    if (!strcmp(cmd, "geometry") && argc == 2) return geometry();
    if (!strcmp(cmd, "walk") && argc == 3) return walk(strtoull(argv[2], nullptr, 10));
    if (!strcmp(cmd, "sizing") && (argc == 8 || argc == 12)) {
        int v[10] = {0};
        for (int k = 0; k < argc - 2; ++k) v[k] = atoi(argv[2 + k]);
        CertKnobs knobs;
        knobs.list = v[6]; knobs.ch = v[7]; knobs.no_small = v[8] != 0; knobs.no_cone = v[9] != 0;
        const CertSizing s = cert_sizing(v[0], v[1], v[2], v[3], v[4], v[5], knobs);
        printf("rc=%d\nerror=%s\nHc=%d Wc=%d CH=%d maxc=%d maxf=%d max_crops=%d nchunks=%d budget=%d small=%d cone=%d\n", s.rc, s.msg, s.Hc, s.Wc, s.CH, s.maxc,
               s.maxf, s.max_crops, s.nchunks, s.budget, s.small, (int)s.cone);
        return 0;
    }
    fprintf(stderr, "usage: %s names | geometry | walk SEED | sizing H W MAX_BATCH N_OUT CROP MAXC [LIST CH NO_SMALL NO_CONE]\n", argv[0]);
    return 2;
}
