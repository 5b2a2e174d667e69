// Stand-alone check of mamdr_amd/csrc/wave_exchange.h (tests/test_gpu_wave_exchange.py builds and runs it once): every
// helper's VALU form against its `__shfl` reference, bit pattern by bit pattern, over all 64 lanes of one wave.
//
// Vectors (64 lanes each, one distinct bit pattern per lane so that a wrong pairing shows): random floats of mixed sign and
// magnitude; the same mixed with +-0 and denormals; with +inf; with +inf and -inf; with ONE NaN (its own payload, at each
// of several lanes); and "all kinds" -- NaNs of 24 different payloads and both signs beside +-0, denormals, +-inf and
// finite values.  The exchanges (wave_xor_get, wave_gather_rows16) move values and are compared on every vector.  The
// second factor of wave_xor_dot64 is the first (finite) vector.  The
// sums are compared on every vector but "all kinds": with two different NaNs among the operands of an addition the payload
// that survives depends on which operand the instruction names first, which C++ fixes in neither form (x + y may be
// emitted as y + x) -- with at most one NaN payload in the wave (inf - inf produces one and the same default NaN wherever
// it happens) the result does not depend on that.
// Exit status: 0 all equal, 1 a mismatch (reported per helper), 2 a HIP error.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "wave_exchange.h"

using namespace mamdr;

constexpr int N_OUT = 2 * (6 + 6 + 2 + 4 + 1);  // (VALU, reference) x (get x 6, add x 6, sum64, sum_16_32, gather x 4, dot64)

template <int O>
__device__ void steps(float x, float* o, int& k, int stride) {
    o[(k++) * stride] = wave_xor_get<O>(x);
    o[(k++) * stride] = wave_xor_get_ref<O>(x);
    o[(k++) * stride] = wave_xor_add<O>(x);
    o[(k++) * stride] = wave_xor_add_ref<O>(x);
}

// one wave per vector: out[v][slot][lane]
__global__ __launch_bounds__(64) void k_check(const float* in, float* out) {
    const int lane = threadIdx.x, v = blockIdx.x;
    const float x = in[v * 64 + lane];
    float* o = out + (size_t)v * N_OUT * 64 + lane;
    int k = 0;
    steps<1>(x, o, k, 64);
    steps<2>(x, o, k, 64);
    steps<4>(x, o, k, 64);
    steps<8>(x, o, k, 64);
    steps<16>(x, o, k, 64);
    steps<32>(x, o, k, 64);
    o[(k++) * 64] = wave_xor_sum64(x);
    o[(k++) * 64] = wave_xor_sum64_ref(x);
    o[(k++) * 64] = wave_xor_sum_16_32(x);
    o[(k++) * 64] = wave_xor_sum_16_32_ref(x);
    float g[4], gr[4];
    wave_gather_rows16(x, g);
    wave_gather_rows16_ref(x, gr);
    for (int q = 0; q < 4; ++q) {
        o[(k++) * 64] = g[q];
        o[(k++) * 64] = gr[q];
    }
    const float y = in[lane];                    // (the second factor: vector 0, finite)
    o[(k++) * 64] = wave_xor_dot64(x, y);
    o[(k++) * 64] = wave_xor_dot64_ref(x, y);
}

static uint32_t rng_state = 0x9e3779b9u;
static uint32_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}
// a finite, normal float of random sign, exponent in [2^-20, 2^20) and random mantissa: distinct with near certainty
static uint32_t rnd_finite() { return (rnd() & 0x807fffffu) | ((107u + rnd() % 40u) << 23); }

#define HIP_OK(e)                                                                \
    do {                                                                         \
        const hipError_t e_ = (e);                                               \
        if (e_ != hipSuccess) {                                                  \
            fprintf(stderr, "HIP error %s at line %d\n", hipGetErrorString(e_), __LINE__); \
            return 2;                                                            \
        }                                                                        \
    } while (0)

int main() {
    std::vector<uint32_t> in;
    std::vector<int> sums_compared;          // per vector: 1 = the sums are compared as well
    auto add_vec = [&](const uint32_t (&x)[64], int sums) {
        in.insert(in.end(), x, x + 64);
        sums_compared.push_back(sums);
    };
    uint32_t x[64];
    for (int rep = 0; rep < 4; ++rep) {                            // random finite floats
        for (int l = 0; l < 64; ++l) x[l] = rnd_finite();
        add_vec(x, 1);
    }
    for (int rep = 0; rep < 2; ++rep) {                            // ... mixed with +-0 and denormals of both signs
        for (int l = 0; l < 64; ++l) x[l] = rnd_finite();
        x[(5 + 31 * rep) & 63] = 0x00000000u;
        x[(20 + 31 * rep) & 63] = 0x80000000u;
        for (int j = 0; j < 12; ++j) x[(3 + 5 * j + rep) & 63] = (rnd() & 0x807fffffu) | (1u + j);      // exponent 0
        add_vec(x, 1);
    }
    for (int rep = 0; rep < 2; ++rep) {                            // denormals only: sums that stay denormal
        for (int l = 0; l < 64; ++l) x[l] = ((rnd() & 0x8000ffffu) | (uint32_t)(l + 1) << 16) & 0x807fffffu;
        add_vec(x, 1);
    }
    for (int lane_inf = 0; lane_inf < 64; lane_inf += 21) {        // one +inf; one -inf; both
        for (int l = 0; l < 64; ++l) x[l] = rnd_finite();
        x[lane_inf] = 0x7f800000u;
        add_vec(x, 1);
        x[lane_inf] = 0xff800000u;
        add_vec(x, 1);
        x[63 - lane_inf] = 0x7f800000u;
        add_vec(x, 1);
    }
    for (int lane_nan = 0; lane_nan < 64; lane_nan += 9) {         // ONE NaN with a payload of its own (quiet or signalling)
        for (int l = 0; l < 64; ++l) x[l] = rnd_finite();
        x[lane_nan] = (lane_nan & 1 ? 0xffc00000u : 0x7f800000u) | (0x1234u + 77u * lane_nan);
        add_vec(x, 1);
    }
    for (int rep = 0; rep < 2; ++rep) {                            // all kinds: the exchanges only
        for (int l = 0; l < 64; ++l) x[l] = rnd_finite();
        for (int j = 0; j < 24; ++j)
            x[(7 * j + 3 * rep) & 63] = (j & 1 ? 0xff800000u : 0x7f800000u) | (j & 2 ? 0x00400000u : 0u) | (0x101u * (j + 1) + rep);
        x[(1 + rep) & 63] = 0x7f800000u;
        x[(2 + rep) & 63] = 0xff800000u;
        x[(8 + rep) & 63] = 0x00000000u;
        x[(15 + rep) & 63] = 0x80000000u;
        x[(22 + rep) & 63] = 0x00000001u;
        x[(29 + rep) & 63] = 0x807fffffu;
        add_vec(x, 0);
    }
    const int n_vec = (int)sums_compared.size();
    for (int v = 0; v < n_vec; ++v)                                // one distinct value per lane
        for (int a = 0; a < 64; ++a)
            for (int b = a + 1; b < 64; ++b)
                if (in[v * 64 + a] == in[v * 64 + b]) {
                    fprintf(stderr, "vector %d: lanes %d and %d hold the same bits\n", v, a, b);
                    return 2;
                }

    float *d_in = nullptr, *d_out = nullptr;
    const size_t out_words = (size_t)n_vec * N_OUT * 64;
    HIP_OK(hipMalloc(&d_in, in.size() * 4));
    HIP_OK(hipMalloc(&d_out, out_words * 4));
    HIP_OK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemset(d_out, 0x5a, out_words * 4));
    hipLaunchKernelGGL(k_check, dim3(n_vec), dim3(64), 0, 0, d_in, d_out);
    HIP_OK(hipGetLastError());
    HIP_OK(hipDeviceSynchronize());
    std::vector<uint32_t> out(out_words);
    HIP_OK(hipMemcpy(out.data(), d_out, out_words * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipFree(d_in));
    HIP_OK(hipFree(d_out));

    static const char* names[N_OUT / 2] = {"wave_xor_get<1>",  "wave_xor_add<1>",  "wave_xor_get<2>",  "wave_xor_add<2>",  "wave_xor_get<4>",
                                           "wave_xor_add<4>",  "wave_xor_get<8>",  "wave_xor_add<8>",  "wave_xor_get<16>", "wave_xor_add<16>",
                                           "wave_xor_get<32>", "wave_xor_add<32>", "wave_xor_sum64",   "wave_xor_sum_16_32", "wave_gather_rows16[0]",
                                           "wave_gather_rows16[1]", "wave_gather_rows16[2]", "wave_gather_rows16[3]", "wave_xor_dot64"};
    static const int is_sum[N_OUT / 2] = {0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 1, 0, 0, 0, 0, 1};
    static const int get_off[6] = {1, 2, 4, 8, 16, 32};
    int bad = 0;
    for (int h = 0; h < N_OUT / 2; ++h) {
        int compared = 0, differ = 0, first_v = -1, first_l = -1, ref_wrong = 0;
        for (int v = 0; v < n_vec; ++v) {
            if (is_sum[h] && !sums_compared[v]) continue;
            const uint32_t* got = &out[((size_t)v * N_OUT + 2 * h) * 64];
            const uint32_t* ref = got + 64;
            for (int l = 0; l < 64; ++l) {
                ++compared;
                if (got[l] != ref[l]) {
                    if (!differ) first_v = v, first_l = l;
                    ++differ;
                }
                // the references themselves, where the host knows the answer: a pure move of the input's bits
                if (!is_sum[h] && h < 12 && ref[l] != in[v * 64 + (l ^ get_off[h / 2])]) ++ref_wrong;
                if (h >= 14 && h < 18 && ref[l] != in[v * 64 + (l & 15) + 16 * (h - 14)]) ++ref_wrong;
            }
        }
        printf("%-24s %5d lane values compared, %d differ from the __shfl form, %d reference values wrong", names[h], compared, differ,
               ref_wrong);
        if (differ) {
            const size_t at = ((size_t)first_v * N_OUT + 2 * h) * 64 + first_l;
            printf("  (first: vector %d lane %d VALU 0x%08x __shfl 0x%08x)", first_v, first_l, out[at], out[at + 64]);
        }
        printf("\n");
        bad += differ + ref_wrong;
    }
    printf("%s\n", bad ? "MISMATCH" : "ALL EQUAL");
    return bad ? 1 : 0;
}
