// frcnn_host.h -- the host-side plumbing the launchers share, one copy each: the workspace carver, the workspace-size check, the
// declarations of every op's workspace size, the CU count of the current device and the opt-in to more than 64 KB of LDS.
// Host code only ("Host plumbing"): nothing here is a layout a kernel sees, so nothing here is part of the layout stamp.
#pragma once
#include "frcnn_common.h"
#include <atomic>

// Carves a workspace into pieces that each start on a 256-byte boundary.  A null workspace addresses nothing and only counts, so an
// op's ONE layout function serves its size query and its entry point.  Two modes:
//   WsCarver(ws)            the caller's base is 256-byte aligned already (the arena's blocks are): bytes() = the pieces.
//   WsCarver::any_base(ws)  any base address: the first piece lies at align_up(ws, 256) and bytes() holds 256 bytes of slack for it.
struct WsCarver {
    char *base;                          // where the first piece lies; nullptr: count only
    size_t o, slack;                     // the pieces so far; what the move to an aligned base may cost
    explicit WsCarver(void *ws) : base((char *)ws), o(0), slack(0) {}
    static WsCarver any_base(void *ws)
    {
        WsCarver c(ws ? (char *)ws + (align_up((uintptr_t)ws, 256) - (uintptr_t)ws) : nullptr);
        c.slack = 256;
        return c;
    }
    char *here() const { return base ? base + o : nullptr; }             // where the next piece will start
    void *take(size_t bytes)
    {
        void *r = here();
        o += align_up(bytes, 256);
        return r;
    }
    template <class T> T *get(size_t count) { return (T *)take(count * sizeof(T)); }
    size_t bytes() const { return slack + o; }
};

#define FRCNN_REQUIRE_WS(op, have, need)                                                   \
    do {                                                                                   \
        const size_t _have = (have), _need = (need);                                       \
        if (_have < _need) return frcnn_set_error(FRCNN_ERR_WORKSPACE, "%s: workspace %zu < %zu bytes", op, _have, _need); \
    } while (0)

// What frcnn_workspace_bytes() answers per op; each is the total of that op's layout function, next to its entry point.
size_t frcnn_ws_topk(int64_t N);
size_t frcnn_ws_nms(int64_t K);
size_t frcnn_ws_rpn_targets(int64_t N, int64_t G);
size_t frcnn_ws_head_targets(int64_t n);
size_t frcnn_ws_region_proposal(int64_t N, int64_t K, int64_t P);
size_t frcnn_ws_preprocess(int64_t in_hw, int64_t out_hw);
size_t frcnn_ws_head_bwd(int64_t C);
size_t frcnn_ws_rpn_conv(void);
size_t frcnn_ws_rpn_conv_wgrad(void);
size_t frcnn_ws_rpn_conv_f32(int64_t C);
size_t frcnn_ws_detect(int64_t P, int64_t C);
size_t frcnn_ws_eval(int64_t D, int64_t G);
size_t frcnn_ws_coco_eval(int64_t D, int64_t G);
size_t frcnn_ws_eval_merge(int64_t n1, int64_t n2);
size_t frcnn_ws_coco_eval_pooled(int64_t D, int64_t G);
size_t frcnn_ws_detect_merge(int64_t out_capacity, int64_t C);

// CUs of the current device (cached per device index below 64); 0 when there is no current device or the query fails -- what a
// launcher does then is the launcher's business.
int frcnn_cu_count();
static inline int frcnn_cu_count_or(int fallback) { const int n = frcnn_cu_count(); return n > 0 ? n : fallback; }

// More than 64 KB of dynamic LDS is an opt-in per (function, device): done[64] remembers the devices that have it (one array per kernel).
int frcnn_reserve_lds(const void *kernel, size_t bytes, const char *who, std::atomic<unsigned char> *done);
