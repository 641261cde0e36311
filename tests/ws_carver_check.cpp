// ws_carver_check.cpp -- the workspace carver of csrc/frcnn_host.h on its own, against arithmetic written out by hand (never against a
// second run of itself).  A stand-alone host program: tests/test_ws_carver_host.py compiles and runs it; it also builds with
// -fsanitize=address,undefined.  Prints one line per failed check and exits 1, or "ws_carver_check: N checks OK" and exits 0.
#include "frcnn_host.h"
#include <cstdio>
#include <cstdlib>
#include <vector>

static int g_checks = 0, g_failed = 0;
#define CHECK(cond)                                                                        \
    do {                                                                                   \
        ++g_checks;                                                                        \
        if (!(cond)) { ++g_failed; std::printf("FAILED line %d: %s\n", __LINE__, #cond); } \
    } while (0)

static size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct Piece { char *p; size_t bytes; };

// pieces lie in order, each on a 256-byte boundary, none reaching into the next, the last one ending inside [lo, hi)
static void check_pieces(const std::vector<Piece> &v, char *lo, char *hi)
{
    for (size_t i = 0; i < v.size(); ++i) {
        CHECK(((uintptr_t)v[i].p & 255) == 0);
        CHECK(v[i].p >= lo && v[i].p + v[i].bytes <= hi);
        if (i + 1 < v.size()) CHECK(v[i].p + v[i].bytes <= v[i + 1].p);
    }
}

// the VOC evaluator's layout (csrc/eval.hip): ticket line | winner words [16][G] u64 | match [D] i32 | reach [D] u32
static void eval_layout(int64_t D, int64_t G, void *ws, std::vector<Piece> *v, size_t *total)
{
    WsCarver c = WsCarver::any_base(ws);
    v->push_back({(char *)c.get<int32_t>(16), 64});
    v->push_back({(char *)c.get<unsigned long long>((size_t)16 * G), (size_t)16 * G * 8});
    v->push_back({(char *)c.get<int32_t>((size_t)D), (size_t)D * 4});
    v->push_back({(char *)c.get<uint32_t>((size_t)D), (size_t)D * 4});
    *total = c.bytes();
}

// the detection post-process (csrc/detect.hip), n = (C - 1) P: boxes [n] float4 | scores [n] f32 | kept rows [n] i32 | counts [C-1] i32
static void detect_layout(int64_t P, int64_t C, void *ws, std::vector<Piece> *v, size_t *total)
{
    const size_t n = (size_t)(C - 1) * (size_t)P;
    WsCarver c = WsCarver::any_base(ws);
    v->push_back({(char *)c.take(n * 16), n * 16});
    v->push_back({(char *)c.get<float>(n), n * 4});
    v->push_back({(char *)c.get<int32_t>(n), n * 4});
    v->push_back({(char *)c.get<int32_t>((size_t)(C - 1)), (size_t)(C - 1) * 4});
    *total = c.bytes();
}

int main()
{
    std::vector<char> mem(1 << 20);
    char *b = (char *)up256((uintptr_t)mem.data());                     // a 256-byte aligned address with > 1 MB - 256 behind it

    {   // plain mode: pieces of 1, 0, 256, 257 bytes and a typed one
        const size_t sizes[] = {1, 0, 256, 257, 3 * sizeof(double)};
        const size_t at[] = {0, 256, 256, 512, 1024};                   // a 0-byte piece takes no room: the next piece starts where it does
        WsCarver n(nullptr), r(b);
        for (int i = 0; i < 5; ++i) {
            CHECK(n.here() == nullptr && r.here() == b + at[i]);
            void *pn = i < 4 ? n.take(sizes[i]) : (void *)n.get<double>(3);
            void *pr = i < 4 ? r.take(sizes[i]) : (void *)r.get<double>(3);
            CHECK(pn == nullptr && pr == b + at[i]);
        }
        CHECK(n.bytes() == 1280 && r.bytes() == 1280);                  // 256 + 0 + 256 + 512 + 256: null base and real base agree
        CHECK(WsCarver(nullptr).bytes() == 0 && WsCarver::any_base(nullptr).bytes() == 256);
    }

    const int64_t eval_DG[][2] = {{6000, 64}, {1, 1}, {63, 3}, {64, 1024}, {522240, 1024}};
    for (const auto &dg : eval_DG) {
        const int64_t D = dg[0], G = dg[1];
        const size_t plain = 256 + up256((size_t)16 * G * 8) + up256((size_t)D * 4) + up256((size_t)D * 4);
        std::vector<Piece> v;
        size_t total = 0;
        eval_layout(D, G, nullptr, &v, &total);
        CHECK(total == 256 + plain);
        for (const Piece &p : v) CHECK(p.p == nullptr);
        if (256 + plain + 255 > mem.size() - 256) continue;             // the largest shape: size only
        for (int k : {0, 1, 64, 255}) {
            v.clear();
            size_t t2 = 0;
            eval_layout(D, G, b + k, &v, &t2);
            char *first = (char *)up256((uintptr_t)(b + k));
            CHECK(t2 == total);
            CHECK(v[0].p == first);
            CHECK(v[1].p == first + 256 && v[2].p == v[1].p + up256((size_t)16 * G * 8) && v[3].p == v[2].p + up256((size_t)D * 4));
            check_pieces(v, b + k, b + k + t2);
        }
    }

    const int64_t det_PC[][2] = {{300, 21}, {1, 2}, {3, 2}, {17, 256}, {2048, 256}};
    for (const auto &pc : det_PC) {
        const int64_t P = pc[0], C = pc[1];
        const size_t n = (size_t)(C - 1) * (size_t)P;
        const size_t plain = up256(n * 16) + up256(n * 4) + up256(n * 4) + up256((size_t)(C - 1) * 4);
        std::vector<Piece> v;
        size_t total = 0;
        detect_layout(P, C, nullptr, &v, &total);
        CHECK(total == 256 + plain);
        if (256 + plain + 255 > mem.size() - 256) continue;
        for (int k : {0, 1, 64, 255}) {
            v.clear();
            size_t t2 = 0;
            detect_layout(P, C, b + k, &v, &t2);
            char *first = (char *)up256((uintptr_t)(b + k));
            CHECK(t2 == total);
            CHECK(v[0].p == first && v[1].p == first + up256(n * 16) && v[2].p == v[1].p + up256(n * 4) && v[3].p == v[2].p + up256(n * 4));
            check_pieces(v, b + k, b + k + t2);
        }
    }

    if (g_failed) { std::printf("ws_carver_check: %d of %d checks FAILED\n", g_failed, g_checks); return 1; }
    std::printf("ws_carver_check: %d checks OK\n", g_checks);
    return 0;
}
