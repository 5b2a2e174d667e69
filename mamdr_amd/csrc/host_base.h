// What host code without HIP (retrieval_host.h, which the host compiler alone builds) shares with the rest: the sizes of a
// retrieval call that its driver and its kernels (mamdr_kernels.h) both read, the error buffer behind *_last_error and the
// pointer-alignment check (host_common.h includes this for both).
#pragma once
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/mamdr_hip.h"

namespace mamdr {

constexpr int REC_TILE = 64;          // candidates per workgroup of k_rec_score (chunks are multiples of it)
constexpr int REC_KMAX = 128;         // largest K
constexpr int REC_QBLOCK = 256;       // queries per pass over the candidates (sizes the workspace)
constexpr int SLATE_WAVE = 64;        // slates of up to this many entries: one wave each

// the text behind mamdr_last_error / mamdr_graph_last_error: one thread_local instance per engine
struct ErrBuf {
    char text[512] = "";
    int fail(int code, const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(text, sizeof(text), fmt, ap);
        va_end(ap);
        return code;
    }
};

// whether one of the pointers is not aligned to its element size, `mask` = that size - 1 (3, 7); a null pointer is aligned
template <typename... P>
inline bool misaligned(uintptr_t mask, const P*... ptrs) {
    return ((... | (uintptr_t)ptrs) & mask) != 0;
}

}  // namespace mamdr
