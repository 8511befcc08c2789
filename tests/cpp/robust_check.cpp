// robust_check.cpp -- host check of the robust mosaic's kernel: k_mosaic_robust (hg_k_robust.hip) itself, compiled for the CPU behind the
// thread-index shim and its wave extension (hip_wave_shim.h: a block is 256 real threads, LDS static storage) and run under AddressSanitizer
// + UndefinedBehaviorSanitizer on exact-size heap buffers: any byte read or written outside a field, a frame, the table, the gains, the
// canvas or the weight plane is reported.  The cases are made here and every result is compared with what this file computes ITSELF from
// the header's steps by sorting each pixel's contributors: every mode and channel count, with and without gains, a frame set with holes,
// empty frames and windows beside the canvas (staged in LDS), a stack of ROB_LMAX + 2 frames over one tile (the walk through global
// memory), one of exactly ROB_LMAX, stacks of 16, 17 and 33 (where a launch takes more slots), frames and canvases at odd addresses, no
// frames at all.  A stand-alone program, no GPU.
#include "hip_wave_shim.h"
#include "hg_k_robust.hip"
using namespace hg;

static uint32_t g_rng = 12345;
static uint32_t rnd() { g_rng = g_rng * 1664525u + 1013904223u; return g_rng >> 8; }

struct Geo { int x, y, w, h; };
struct Case {
    std::vector<Geo> geoms;
    int C, mode, cx, cy, cw, ch, values;                      // values: 0 random bytes, 1 from {0, 127, 128, 255}, 2 two values only
    float trim;
    bool gained, odd;
};
struct Run {
    const MosaicFrame4 *table; int n_frames; const uint8_t *fld, *pix; int mode; float trim; int cx, cy, cw, ch; uint32_t tiles_x;
    uint8_t *canvas; float *weight; const float *gains; int C; uint32_t cap;
};
static void run_block(uint32_t, void *arg)
{
    const Run &r = *(const Run *)arg;
#define ROBUST(CC) k_mosaic_robust<CC>(r.table, r.n_frames, r.fld, r.pix, r.mode, r.trim, r.cap, r.cx, r.cy, r.cw, r.ch, r.tiles_x, r.canvas, r.weight, r.gains)
    switch (r.C) { case 1: ROBUST(1); break; case 2: ROBUST(2); break; case 3: ROBUST(3); break; default: ROBUST(4); break; }
}

// An exact-size heap block whose start is aligned to 16 bytes plus `front`.
static uint8_t *block(size_t front, size_t bytes, int fill, std::vector<void *> &owned)
{
    uint8_t *p = (uint8_t *)malloc(front + bytes + (front + bytes == 0));
    owned.push_back(p);
    memset(p, fill, front + bytes);
    return p + front;
}

// Step 4 of the header from the sorted values.
static uint32_t expect(std::vector<uint32_t> s, int mode, float trim)
{
    const int n = (int)s.size();
    if (n == 0) return 0;
    std::sort(s.begin(), s.end());
    if (mode == 2) return s[0];
    if (mode == 3) return s[n - 1];
    if (mode == 0) return n % 2 ? s[(n - 1) / 2] : (s[n / 2 - 1] + s[n / 2] + 1) >> 1;
    const int t = std::min((int)(trim * (float)n), (n - 1) / 2), m = n - 2 * t;
    uint32_t S = 0;
    for (int k = t; k <= n - 1 - t; k++) S += s[k];
    return (2 * S + m) / (2 * m);
}

static int run_case(int id, const Case &c)
{
    const size_t F = c.geoms.size(), C = (size_t)c.C;
    std::vector<void *> owned;
    std::vector<uint64_t> fo(F), po(F);
    size_t f_end = 0, p_end = 0;
    for (size_t f = 0; f < F; f++) {                            // odd: the fields at odd multiples of 8, the frames at odd byte distances
        const size_t px = (size_t)std::max(c.geoms[f].w, 0) * (size_t)std::max(c.geoms[f].h, 0);
        fo[f] = f_end + (c.odd ? 8 * (2 * f + 1) : 0); po[f] = p_end + (c.odd ? 2 * f + 1 : 0);
        f_end = fo[f] + px * 8; p_end = po[f] + px * C;
    }
    MosaicFrame4 *table = reinterpret_cast<MosaicFrame4 *>(block(0, ((F + 3) / 4) * sizeof(MosaicFrame4), 0, owned));
    float *gains = reinterpret_cast<float *>(block(0, ((F + 3) / 4) * 16, 0, owned));
    for (size_t k = 0; k < ((F + 3) / 4) * 4; k++) gains[k] = 1.0f;
    uint8_t *fld = block(0, f_end, 0, owned), *pix = block(c.odd ? 1 : 0, p_end, 0xEE, owned);
    for (size_t f = 0; f < F; f++) {
        const Geo &g = c.geoms[f];
        table[f / 4].f[f % 4] = MosaicFrame{fo[f], po[f], g.x, g.y, g.w, g.h};
        gains[f] = 0.5f + (float)(rnd() % 1200) / 1000.0f;      // 0.5 .. 1.7: bytes saturate
        const size_t px = (size_t)std::max(g.w, 0) * (size_t)std::max(g.h, 0);
        float *co = reinterpret_cast<float *>(fld + fo[f]);
        for (size_t k = 0; k < px; k++) {
            co[2 * k] = (float)(rnd() % 97) - 3.5f; co[2 * k + 1] = (float)(rnd() % 61) * 0.5f;
            const uint32_t hole = rnd() % 20;
            if (px >= 20 && hole == 0) co[2 * k] = NAN; else if (px >= 20 && hole == 1) co[2 * k + 1] = INFINITY; else if (px >= 20 && hole == 2) co[2 * k] = 1e30f;
            for (size_t ch = 0; ch < C; ch++) {
                static const uint8_t four[4] = {0, 127, 128, 255};
                pix[po[f] + k * C + ch] = c.values == 1 ? four[rnd() & 3] : c.values == 2 ? ((rnd() & 1) ? 201 : 17) : (uint8_t)(rnd() & 255);
            }
        }
    }
    const size_t n_px = (size_t)c.cw * (size_t)c.ch;
    uint8_t *canvas = block(c.odd ? 1 : 0, n_px * C, 0xA5, owned);
    float *weight = reinterpret_cast<float *>(block(0, n_px * 4, 0xA5, owned));
    Run r{F ? table : nullptr, (int)F, fld, pix, c.mode, c.trim, c.cx, c.cy, c.cw, c.ch, (uint32_t)((c.cw + 63) / 64), canvas, weight, c.gained ? gains : nullptr, c.C, rob_cap((int)F)};
    const uint32_t n_blocks = r.tiles_x * (uint32_t)((c.ch + 3) / 4);
    if (!wave_block_run(n_blocks, run_block, &r)) { printf("cannot start a thread\n"); exit(2); }
    int bad = 0, most = 0;
    for (int j = 0; j < c.ch; j++) for (int i = 0; i < c.cw; i++) {
        const int64_t X = (int64_t)c.cx + i, Y = (int64_t)c.cy + j;
        std::vector<uint32_t> vals[4];
        for (size_t f = 0; f < F; f++) {
            const Geo &g = c.geoms[f];
            const int64_t u = X - g.x, v = Y - g.y;
            if (g.w <= 0 || g.h <= 0 || u < 0 || u >= g.w || v < 0 || v >= g.h) continue;
            const size_t k = (size_t)v * (size_t)g.w + (size_t)u;
            float sx, sy;
            memcpy(&sx, fld + fo[f] + k * 8, 4); memcpy(&sy, fld + fo[f] + k * 8 + 4, 4);
            if (!std::isfinite(sx) || !std::isfinite(sy)) continue;
            for (size_t ch = 0; ch < C; ch++) {
                uint32_t x = pix[po[f] + k * C + ch];
                if (c.gained && !(C == 4 && ch == 3)) x = (uint32_t)fminf(255.0f, floorf(gains[f] * (float)x + 0.5f));
                vals[ch].push_back(x);
            }
        }
        most = std::max(most, (int)vals[0].size());
        const size_t at = (size_t)j * (size_t)c.cw + (size_t)i;
        for (size_t ch = 0; ch < C; ch++) {
            const uint32_t want = expect(vals[ch], c.mode, c.trim);
            if (canvas[at * C + ch] != want && bad++ < 4)
                printf("case %d: pixel (%d, %d) channel %d: got %u, want %u of %d contributors\n", id, i, j, (int)ch, canvas[at * C + ch], want, (int)vals[ch].size());
        }
        if (weight[at] != (float)vals[0].size() && bad++ < 4) printf("case %d: pixel (%d, %d): weight %g, want %d\n", id, i, j, weight[at], (int)vals[0].size());
    }
    for (void *p : owned) free(p);
    printf("case %d: C %d mode %d trim %g frames %d blocks %u most contributors %d: %s\n", id, c.C, c.mode, c.trim, (int)F, n_blocks, most, bad ? "WRONG" : "ok");
    return bad;
}

int main()
{
    const std::vector<Geo> mixed = {{0, 0, 20, 14}, {7, 3, 18, 12}, {-5, -4, 12, 9}, {0, 0, 0, 5}, {7, 3, 18, 12}, {22, 10, 1, 9}, {30, -2, 16, 6}, {100, 100, 4, 4},
                                    {3, 12, 25, 1}, {5, 2, 60, 9}, {6, 1, 58, 9}, {4, 3, 61, 7}};
    std::vector<Geo> over, at_cap;                            // one tile hit by more frames than are staged, and by exactly as many
    for (uint32_t f = 0; f < ROB_LMAX + 2; f++) over.push_back(Geo{(int)(f % 3), 0, 70, 6});
    for (uint32_t f = 0; f < ROB_LMAX; f++) at_cap.push_back(Geo{0, (int)(f % 2), 66, 5});
    const float trims[4] = {0.0f, 0.1f, 0.25f, 0.49f};
    int bad = 0, id = 0;
    for (int C = 1; C <= 4; C++)
        for (int mode = 0; mode < 4; mode++) {
            const float trim = trims[(C + mode) % 4];
            bad += run_case(id++, Case{mixed, C, mode, -3, -2, 67, 22, (C + mode) % 3, trim, (C + mode) % 2 == 0, C % 2 == 1});
            bad += run_case(id++, Case{over, C, mode, 0, 0, 72, 6, (C + mode + 1) % 3, trim, (C + mode) % 2 == 1, C % 2 == 0});
        }
    for (int k = 0; k < 4; k++) bad += run_case(id++, Case{at_cap, 1 + k, 1, -1, 0, 68, 5, k % 3, trims[k], k % 2 == 0, true});
    for (int k = 0; k < 4; k++) bad += run_case(id++, Case{over, 4 - k, 1, 0, 1, 65, 4, 1, trims[k], false, false});
    for (int n : {16, 17, 33}) {                              // the frame counts at which a launch takes more slots
        std::vector<Geo> some(at_cap.begin(), at_cap.begin() + n);
        bad += run_case(id++, Case{some, 1 + n % 4, n % 2, 0, 0, 66, 5, 0, 0.25f, n % 2 == 0, false});
    }
    bad += run_case(id++, Case{{}, 3, 0, 5, 5, 65, 5, 0, 0.0f, false, true});
    bad += run_case(id++, Case{{{0, 0, 3, 3}}, 4, 1, 0, 0, 1, 1, 0, 0.25f, true, false});
    if (bad) { printf("%d wrong values\n", bad); return 1; }
    printf("host check ran: %d cases, cap %u\n", id, ROB_LMAX);
    return 0;
}
