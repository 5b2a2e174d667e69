// Drives the three forms of mamdr_amd/csrc/retrieval_host.h's retrieval_call (top-K, ranks, slates: recommend_call, rank_call
// and slates_call below fill a RetCall as the C entry points do) with a backend that only records what it is asked for -- no HIP, the CSR offsets served from a host vector -- and holds the record to what
// a call must do, worked out here by brute force from the per-query list lengths: the query blocks, the candidate passes,
// the block pointers, the list passes, the empty-block rules, the slate scan and the refusals with the texts of the C ABI.
// Built and run by tests/test_retrieval_plan_host.py with the host compiler's address and undefined-behaviour sanitizers.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "retrieval_host.h"

using namespace mamdr;

static int fails = 0;
static long checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++checks;                                         \
        if (!(cond)) {                                    \
            if (fails++ < 20) {                           \
                std::printf("FAIL %s: ", #cond);          \
                std::printf(__VA_ARGS__);                 \
                std::printf("\n");                        \
            }                                             \
        }                                                 \
    } while (0)

enum EvType { READ, FILL, PREPARE, BLOCK, LIST, TOPK, COUNT, ORDER, FINISH };
struct Event {
    EvType type;
    RetCall blk{};              // BLOCK
    struct { int64_t c0; int n_chunk, tiles; bool first, last; } ch{};      // TOPK, COUNT
    int64_t j0 = 0, j1 = 0;     // LIST; ORDER: max_len in j0, any_short in j1
    const void* ptr = nullptr;  // FILL
    int byte = 0;
    size_t bytes = 0;
};

struct Recorder {
    int n_item = 1000, n_domain = 3, rec_chunk = 64;
    bool is_ready = true;
    std::vector<int64_t> off;       // what the "device" holds behind d_off
    const int64_t* d_off = nullptr;
    ErrBuf e;
    ErrBuf& err = e;
    RetCall call{};
    std::vector<Event> ev;

    int ready() { return is_ready ? 0 : e.fail(MAMDR_ESTATE, "state incomplete"); }
    int read_back(int64_t* host, const int64_t* dev, size_t n) {
        Event x{READ};
        ev.push_back(x);
        if (dev != d_off || n > off.size()) return e.fail(MAMDR_EHIP, "read-back of %zu offsets from a foreign pointer", n);
        std::memcpy(host, off.data(), n * sizeof(int64_t));
        return MAMDR_OK;
    }
    int fill(void* dev, int byte, size_t bytes) {
        Event x{FILL};
        x.ptr = dev;
        x.byte = byte;
        x.bytes = bytes;
        ev.push_back(x);
        return MAMDR_OK;
    }
    int prepare(const RetCall& r) {
        call = r;
        Event x{PREPARE};
        ev.push_back(x);
        return MAMDR_OK;
    }
    void begin_block(const RetCall& b) {
        Event x{BLOCK};
        x.blk = b;
        ev.push_back(x);
    }
    int list_pass(int64_t j0, int64_t j1) {
        Event x{LIST};
        x.j0 = j0;
        x.j1 = j1;
        ev.push_back(x);
        return MAMDR_OK;
    }
    int cand_pass(int64_t c0, int n_chunk, int tiles, bool first, bool last) {
        Event x{call.kind == RET_TOPK ? TOPK : COUNT};
        x.ch = {c0, n_chunk, tiles, first, last};
        ev.push_back(x);
        return MAMDR_OK;
    }
    void slate_order(int64_t max_len, bool any_short) {
        Event x{ORDER};
        x.j0 = max_len;
        x.j1 = any_short;
        ev.push_back(x);
    }
    int finish() {
        Event x{FINISH};
        ev.push_back(x);
        return MAMDR_OK;
    }
};

// the three forms, filled as the C entry points fill them
static int recommend_call(Recorder& b, const char* fn, bool per_query, int32_t domain, int32_t n_query, const int32_t* d_uid,
                          const int32_t* d_domain, const int32_t* d_cand, int64_t n_cand, const int64_t* d_excl_off,
                          const int32_t* d_excl_ids, int32_t k, int32_t* d_ids_out, float* d_scores_out, float* d_scores_all) {
    RetCall r{RET_TOPK, fn};
    if (per_query) r.per_query = true, r.dom = d_domain;
    else r.domain = domain;
    r.n_query = n_query, r.uid = d_uid, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids;
    r.k = k, r.ids_out = d_ids_out, r.scores_out = d_scores_out, r.scores_all = d_scores_all;
    return retrieval_call(b, r);
}
static int rank_call(Recorder& b, const char* fn, int32_t domain, int32_t n_query, const int32_t* d_uid, const int32_t* d_cand,
                     int64_t n_cand, const int64_t* d_excl_off, const int32_t* d_excl_ids, const int64_t* d_tgt_off,
                     const int32_t* d_tgt_ids, int32_t* d_rank_out, float* d_score_out, int32_t* d_live_out) {
    RetCall r{RET_RANK, fn};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.cand = d_cand, r.n_cand = n_cand;
    r.excl_off = d_excl_off, r.excl_ids = d_excl_ids, r.list_off = d_tgt_off, r.list_ids = d_tgt_ids;
    r.rank_out = d_rank_out, r.score_out = d_score_out, r.live_out = d_live_out;
    return retrieval_call(b, r);
}
static int slates_call(Recorder& b, const char* fn, int32_t domain, int32_t n_query, const int32_t* d_uid, const int64_t* d_slate_off,
                       const int32_t* d_slate_ids, float* d_score_out, int32_t* d_pos_out, int32_t* d_order_out) {
    RetCall r{RET_SLATES, fn};
    r.domain = domain, r.n_query = n_query, r.uid = d_uid, r.list_off = d_slate_off, r.list_ids = d_slate_ids;
    r.score_out = d_score_out, r.pos_out = d_pos_out, r.order_out = d_order_out;
    return retrieval_call(b, r);
}

// the arrays a call points at: real memory, large enough for every shape below (the driver only offsets the pointers)
struct Arrays {
    std::vector<int32_t> uid, dom, cand, excl_ids, ids_out, list_ids, rank_out, live_out, pos_out, order_out;
    std::vector<float> scores_out, scores_all, score_out;
    std::vector<int64_t> excl_off, list_off;
    Arrays() {
        const size_t nq = 520, nc = 300, nl = 520 * 257;
        uid.resize(nq), dom.resize(nq), cand.resize(nc), excl_ids.resize(8), ids_out.resize(nq * 128), list_ids.resize(nl);
        rank_out.resize(nl), live_out.resize(nq), pos_out.resize(nl), order_out.resize(nl);
        scores_out.resize(nq * 128), scores_all.resize(nq * nc), score_out.resize(nl);
        excl_off.resize(nq + 1), list_off.resize(nq + 1);
    }
};
static Arrays A;

// ---- the shapes
static const int32_t N_QUERY[] = {1, 255, 256, 257, 513};
static const int REC_CHUNKS[] = {64, 128};
static std::vector<int64_t> cand_counts(int chunk) { return {1, 63, 64, 65, chunk, chunk + 1, 2 * chunk + 1}; }
static const int64_t LENS[] = {0, 1, 63, 64, 65, 257};
// per-query list lengths: 0 every length in turn, 1 the first block without entries, 2 the last block without entries,
// 3 no entries at all, 4 every length in turn but block 0 with 257-entry and empty slates only (no short slate beside long ones)
static std::vector<int64_t> lengths(int32_t n_query, int pattern) {
    std::vector<int64_t> len((size_t)n_query);
    const int32_t last_block = (n_query - 1) / 256 * 256;
    for (int32_t q = 0; q < n_query; ++q) {
        int64_t l = LENS[(q * 7 + q / 6) % 6];
        if (pattern == 1 && q < 256) l = 0;
        if (pattern == 2 && q >= last_block) l = 0;
        if (pattern == 3) l = 0;
        if (pattern == 4 && q < 256) l = q % 3 == 0 ? 257 : 0;
        len[(size_t)q] = l;
    }
    return len;
}
static std::vector<int64_t> csr(const std::vector<int64_t>& len) {
    std::vector<int64_t> off(len.size() + 1, 0);
    for (size_t q = 0; q < len.size(); ++q) off[q + 1] = off[q] + len[q];
    return off;
}

// ---- what every call's record must show
// the BLOCK events tile [0, n_query) in order, at most 256 queries each, with the call's pointers offset to the block
static void check_block(const Recorder& b, const Event& x, int32_t want_qb, const char* what) {
    const RetCall& r = b.call;
    const RetCall& k = x.blk;
    const int32_t qb = want_qb;         // (the uid check below holds the block to it)
    CHECK(k.n_query >= 1 && k.n_query <= 256 && qb + k.n_query <= r.n_query, "%s: block [%d, +%d) of %d", what, qb, k.n_query, r.n_query);
    const int32_t rest = r.n_query - want_qb;
    CHECK(k.n_query == (rest < 256 ? rest : 256), "%s: block of %d queries with %d left", what, k.n_query, rest);
    CHECK(k.uid == r.uid + qb, "%s: uid", what);
    CHECK(k.dom == (r.dom ? r.dom + qb : nullptr), "%s: dom", what);
    CHECK(k.excl_off == (r.excl_off ? r.excl_off + qb : nullptr), "%s: excl_off", what);
    CHECK(k.ids_out == (r.ids_out ? r.ids_out + (size_t)qb * r.k : nullptr), "%s: ids_out", what);
    CHECK(k.scores_out == (r.scores_out ? r.scores_out + (size_t)qb * r.k : nullptr), "%s: scores_out", what);
    CHECK(k.scores_all == (r.scores_all ? r.scores_all + (size_t)qb * r.n_cand : nullptr), "%s: scores_all", what);
    CHECK(k.list_off == (r.list_off ? r.list_off + qb : nullptr), "%s: list_off", what);
    CHECK(k.live_out == (r.live_out ? r.live_out + qb : nullptr), "%s: live_out", what);
    // what is not per query stays the call's
    CHECK(k.kind == r.kind && k.fn == r.fn && k.domain == r.domain && k.cand == r.cand && k.n_cand == r.n_cand && k.chunk == r.chunk &&
              k.excl_ids == r.excl_ids && k.k == r.k && k.list_ids == r.list_ids && k.n_list == r.n_list && k.score_out == r.score_out &&
              k.rank_out == r.rank_out && k.pos_out == r.pos_out && k.order_out == r.order_out,
          "%s: the block's call-wide fields", what);
}
// events [i, ...) of type `t`: candidate passes that tile [0, n_cand) exactly once; -> the first event behind them
static size_t check_passes(const Recorder& b, size_t i, EvType t, int64_t n_cand, const char* what) {
    std::vector<int> seen((size_t)n_cand, 0);
    size_t n_pass = 0, first_i = i;
    int64_t next = 0;
    for (; i < b.ev.size() && b.ev[i].type == t; ++i, ++n_pass) {
        const auto& c = b.ev[i].ch;
        CHECK(c.c0 == next, "%s: pass at %lld, expected %lld", what, (long long)c.c0, (long long)next);
        CHECK(c.n_chunk >= 1 && c.n_chunk <= b.rec_chunk && c.c0 + c.n_chunk <= n_cand, "%s: pass [%lld, +%d) of %lld, chunk %d", what,
              (long long)c.c0, c.n_chunk, (long long)n_cand, b.rec_chunk);
        int tiles = 0;
        for (int p = 0; p < c.n_chunk; p += 64) ++tiles;
        CHECK(c.tiles == tiles, "%s: %d tiles for %d candidates", what, c.tiles, c.n_chunk);
        for (int64_t p = c.c0; p < c.c0 + c.n_chunk && p < n_cand; ++p) seen[(size_t)p] += 1;
        next = c.c0 + c.n_chunk;
    }
    // the chunk rule and the number of passes, by counting: tiles of 64 until the candidates or rec_chunk are covered
    int want_chunk = 0;
    while (want_chunk < n_cand && want_chunk < b.rec_chunk) want_chunk += 64;
    size_t want_pass = 0;
    for (int64_t p = 0; p < n_cand; p += want_chunk) ++want_pass;
    CHECK(b.call.chunk == want_chunk, "%s: chunk %d, expected %d", what, b.call.chunk, want_chunk);
    CHECK(n_pass == want_pass, "%s: %zu candidate passes, expected %zu", what, n_pass, want_pass);
    for (size_t k = first_i; k < i; ++k) {
        CHECK(b.ev[k].ch.first == (k == first_i), "%s: first flag of pass %zu", what, k - first_i);
        CHECK(b.ev[k].ch.last == (k + 1 == i), "%s: last flag of pass %zu", what, k - first_i);
    }
    for (int64_t p = 0; p < n_cand; ++p) CHECK(seen[(size_t)p] == 1, "%s: candidate %lld covered %d times", what, (long long)p, seen[(size_t)p]);
    return i;
}

static long walk_topk(int32_t n_query, int chunk, int64_t n_cand, bool per_query, bool with_list) {
    Recorder b;
    b.rec_chunk = chunk;
    b.n_item = (int)n_cand;          // without a list the catalogue is the candidate list
    const int32_t k = 1 + (int32_t)((n_query + n_cand) % 128);
    const int rc = recommend_call(b, "fn", per_query, 1, n_query, A.uid.data(), per_query ? A.dom.data() : nullptr,
                                  with_list ? A.cand.data() : nullptr, with_list ? n_cand : -5, A.excl_off.data(), A.excl_ids.data(), k,
                                  A.ids_out.data(), A.scores_out.data(), A.scores_all.data());
    char what[96];
    std::snprintf(what, sizeof(what), "top-K n_query %d chunk %d n_cand %lld", n_query, chunk, (long long)n_cand);
    CHECK(rc == MAMDR_OK, "%s: %d %s", what, rc, b.e.text);
    if (rc != MAMDR_OK || b.ev.empty()) return 1;
    CHECK(b.ev[0].type == PREPARE, "%s: first event %d", what, (int)b.ev[0].type);
    CHECK(b.call.kind == RET_TOPK && b.call.n_cand == n_cand && b.call.domain == (per_query ? -1 : 1) && b.call.k == k, "%s: call record", what);
    CHECK(b.call.uid == A.uid.data() && b.call.dom == (per_query ? A.dom.data() : nullptr) && b.call.excl_off == A.excl_off.data() &&
              b.call.excl_ids == A.excl_ids.data() && b.call.cand == (with_list ? A.cand.data() : nullptr) &&
              b.call.ids_out == A.ids_out.data() && b.call.scores_out == A.scores_out.data() && b.call.scores_all == A.scores_all.data(),
          "%s: the call's pointers", what);
    size_t i = 1;
    int32_t qb = 0;
    while (i < b.ev.size() && b.ev[i].type == BLOCK) {
        check_block(b, b.ev[i], qb, what);
        qb += b.ev[i].blk.n_query;
        i = check_passes(b, i + 1, TOPK, n_cand, what);
    }
    CHECK(qb == n_query, "%s: blocks end at %d", what, qb);
    CHECK(i + 1 == b.ev.size() && b.ev[i].type == FINISH, "%s: the record ends with event %zu of %zu", what, i, b.ev.size());
    return 1;
}

static long walk_rank(int32_t n_query, int chunk, int64_t n_cand, int pattern) {
    Recorder b;
    b.rec_chunk = chunk;
    const std::vector<int64_t> len = lengths(n_query, pattern);
    b.off = csr(len);
    b.d_off = A.list_off.data();
    const int64_t n_tgt = b.off.back();
    const int rc = rank_call(b, "fn", 2, n_query, A.uid.data(), A.cand.data(), n_cand, nullptr, nullptr, A.list_off.data(),
                             A.list_ids.data(), A.rank_out.data(), A.score_out.data(), A.live_out.data());
    char what[96];
    std::snprintf(what, sizeof(what), "ranks n_query %d chunk %d n_cand %lld pattern %d", n_query, chunk, (long long)n_cand, pattern);
    CHECK(rc == MAMDR_OK, "%s: %d %s", what, rc, b.e.text);
    if (rc != MAMDR_OK || b.ev.size() < 3) return 1;
    size_t i = 0;
    CHECK(b.ev[i].type == READ, "%s: event 0", what);
    CHECK(b.ev[++i].type == PREPARE, "%s: event 1", what);
    CHECK(b.call.kind == RET_RANK && b.call.n_list == n_tgt, "%s: %lld targets, expected %lld", what, (long long)b.call.n_list, (long long)n_tgt);
    CHECK(b.call.uid == A.uid.data() && b.call.cand == A.cand.data() && b.call.list_off == A.list_off.data() && b.call.list_ids == A.list_ids.data() &&
              b.call.rank_out == A.rank_out.data() && b.call.score_out == A.score_out.data() && b.call.live_out == A.live_out.data() &&
              b.call.n_cand == n_cand && b.call.domain == 2 && !b.call.excl_off && !b.call.excl_ids,
          "%s: the call's pointers", what);
    ++i;
    if (n_tgt > 0) {
        const Event& f = b.ev[i++];
        CHECK(f.type == FILL && f.ptr == A.rank_out.data() && f.byte == 0 && f.bytes == (size_t)n_tgt * 4, "%s: rank_out is not zeroed", what);
    }
    {
        const Event& f = b.ev[i++];
        CHECK(f.type == FILL && f.ptr == A.live_out.data() && f.byte == 0 && f.bytes == (size_t)n_query * 4, "%s: live_out is not zeroed", what);
    }
    int32_t qb = 0;
    while (i < b.ev.size() && b.ev[i].type == BLOCK) {
        const int32_t n = b.ev[i].blk.n_query;
        check_block(b, b.ev[i], qb, what);
        int64_t j0 = 0, j1 = 0;                 // the block's entries, summed from the lengths
        for (int32_t q = 0; q < qb + n && q < n_query; ++q) (q < qb ? j0 : j1) += len[(size_t)q];
        j1 += j0;
        ++i;
        CHECK(i < b.ev.size() && b.ev[i].type == LIST && b.ev[i].j0 == j0 && b.ev[i].j1 == j1, "%s: list pass of block %d, expected [%lld, %lld)",
              what, qb, (long long)j0, (long long)j1);
        if (i < b.ev.size() && b.ev[i].type == LIST) ++i;
        i = check_passes(b, i, COUNT, n_cand, what);     // for a block without targets too: live_out needs them
        qb += n;
    }
    CHECK(qb == n_query, "%s: blocks end at %d", what, qb);
    CHECK(i + 1 == b.ev.size() && b.ev[i].type == FINISH, "%s: the record ends with event %zu of %zu", what, i, b.ev.size());
    return 1;
}

static long walk_slates(int32_t n_query, int pattern, bool want_order) {
    Recorder b;
    const std::vector<int64_t> len = lengths(n_query, pattern);
    b.off = csr(len);
    b.d_off = A.list_off.data();
    const int64_t n_ent = b.off.back();
    const int rc = slates_call(b, "fn", 0, n_query, A.uid.data(), A.list_off.data(), A.list_ids.data(), A.score_out.data(),
                               A.pos_out.data(), want_order ? A.order_out.data() : nullptr);
    char what[96];
    std::snprintf(what, sizeof(what), "slates n_query %d pattern %d", n_query, pattern);
    CHECK(rc == MAMDR_OK, "%s: %d %s", what, rc, b.e.text);
    if (rc != MAMDR_OK || b.ev.empty()) return 1;
    CHECK(b.ev[0].type == READ, "%s: event 0", what);
    if (n_ent == 0) {                           // done before any workspace is touched
        CHECK(b.ev.size() == 1, "%s: %zu events in a call without entries", what, b.ev.size());
        return 1;
    }
    size_t i = 1;
    CHECK(b.ev[i].type == PREPARE, "%s: event 1", what);
    CHECK(b.call.kind == RET_SLATES && b.call.n_list == n_ent, "%s: %lld entries, expected %lld", what, (long long)b.call.n_list, (long long)n_ent);
    CHECK(b.call.uid == A.uid.data() && b.call.list_off == A.list_off.data() && b.call.list_ids == A.list_ids.data() &&
              b.call.score_out == A.score_out.data() && b.call.pos_out == A.pos_out.data() &&
              b.call.order_out == (want_order ? A.order_out.data() : nullptr) && b.call.domain == 0,
          "%s: the call's pointers", what);
    ++i;
    if (want_order) {
        const Event& f = b.ev[i++];
        CHECK(f.type == FILL && f.ptr == A.order_out.data() && f.byte == 0xff && f.bytes == (size_t)n_ent * 4, "%s: order_out is not filled", what);
    }
    for (int32_t qb = 0; qb < n_query; qb += 256) {
        const int32_t n = n_query - qb < 256 ? n_query - qb : 256;
        int64_t j0 = 0, count = 0, max_len = 0;
        bool any_short = false;
        for (int32_t q = 0; q < qb; ++q) j0 += len[(size_t)q];
        for (int32_t q = qb; q < qb + n; ++q) {
            const int64_t l = len[(size_t)q];
            count += l;
            if (l > max_len) max_len = l;
            if (l >= 1 && l <= 64) any_short = true;
        }
        if (count == 0) continue;               // nothing is issued for a block of empty slates
        CHECK(i + 2 < b.ev.size(), "%s: the record ends inside block %d", what, qb);
        if (i + 2 >= b.ev.size()) return 1;
        CHECK(b.ev[i].type == BLOCK, "%s: block %d does not begin", what, qb);
        check_block(b, b.ev[i], qb, what);
        ++i;
        CHECK(b.ev[i].type == LIST && b.ev[i].j0 == j0 && b.ev[i].j1 == j0 + count, "%s: list pass of block %d", what, qb);
        ++i;
        CHECK(b.ev[i].type == ORDER && b.ev[i].j0 == max_len && (b.ev[i].j1 != 0) == any_short,
              "%s: block %d ordered with max_len %lld any_short %d, expected %lld %d", what, qb, (long long)b.ev[i].j0, (int)b.ev[i].j1,
              (long long)max_len, (int)any_short);
        ++i;
    }
    CHECK(i + 1 == b.ev.size() && b.ev[i].type == FINISH, "%s: the record ends with event %zu of %zu", what, i, b.ev.size());
    return 1;
}

// ---- refusals: code and text as the C ABI gives them (the texts of mamdr_recommend(_domain), mamdr_rank_domain and
// mamdr_rank_slates, `fn` in the place of the entry point's name); nothing but the read-back may precede one
struct Args {       // a well-formed call of every form; a row of the table breaks one thing
    bool per_query = false;
    bool is_ready = true;
    int32_t domain = 1, n_query = 7, k = 5;
    const int32_t *uid = A.uid.data(), *dom = nullptr, *cand = A.cand.data(), *excl_ids = A.excl_ids.data(), *list_ids = A.list_ids.data();
    int64_t n_cand = 70;
    const int64_t *excl_off = A.excl_off.data(), *list_off = A.list_off.data();
    int32_t *ids_out = A.ids_out.data(), *rank_out = A.rank_out.data(), *live_out = A.live_out.data(), *pos_out = A.pos_out.data(),
            *order_out = A.order_out.data();
    float *scores_out = A.scores_out.data(), *scores_all = A.scores_all.data(), *score_out = A.score_out.data();
    std::vector<int64_t> off{0, 2, 2, 5, 6, 6, 9, 10};
};
template <typename T>
static T* shifted(T* p, int bytes) { return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(p) + (uintptr_t)bytes); }

static std::string text(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    return buf;
}
static long rows = 0;
enum Form { TOPK_FORM, RANK_FORM, SLATES_FORM };
static void refuse(Form form, const char* row, const std::function<void(Args&)>& spoil, int code, const std::string& want, bool reads) {
    Args a;
    spoil(a);
    Recorder b;
    b.is_ready = a.is_ready;
    b.off = a.off;
    b.d_off = A.list_off.data();
    int rc;
    if (form == TOPK_FORM)
        rc = recommend_call(b, "fn", a.per_query, a.domain, a.n_query, a.uid, a.dom, a.cand, a.n_cand, a.excl_off, a.excl_ids, a.k, a.ids_out,
                            a.scores_out, a.scores_all);
    else if (form == RANK_FORM)
        rc = rank_call(b, "fn", a.domain, a.n_query, a.uid, a.cand, a.n_cand, a.excl_off, a.excl_ids, a.list_off, a.list_ids, a.rank_out,
                       a.score_out, a.live_out);
    else
        rc = slates_call(b, "fn", a.domain, a.n_query, a.uid, a.list_off, a.list_ids, a.score_out, a.pos_out, a.order_out);
    ++rows;
    CHECK(rc == code, "form %d, %s: code %d, expected %d (%s)", (int)form, row, rc, code, b.e.text);
    CHECK(want == b.e.text, "form %d, %s: text \"%s\", expected \"%s\"", (int)form, row, b.e.text, want.c_str());
    CHECK(b.ev.size() == (reads ? 1u : 0u) && (b.ev.empty() || b.ev[0].type == READ), "form %d, %s: %zu backend calls before the refusal",
          (int)form, row, b.ev.size());
}

static void refusals() {
    const std::string unaligned = "fn: a pointer is not aligned to its element size";
    const std::string excl = "fn: the exclusion lists need both their offsets and their ids";
    // ---- top-K
    const std::string null_dom = "fn: null uid / output pointer", null_pq = "fn: null uid / domain / output pointer";
    refuse(TOPK_FORM, "null uid", [](Args& a) { a.uid = nullptr; }, MAMDR_EINVAL, null_dom, false);
    refuse(TOPK_FORM, "null ids_out", [](Args& a) { a.ids_out = nullptr; }, MAMDR_EINVAL, null_dom, false);
    refuse(TOPK_FORM, "null scores_out", [](Args& a) { a.scores_out = nullptr; }, MAMDR_EINVAL, null_dom, false);
    refuse(TOPK_FORM, "per query, null uid", [](Args& a) { a.per_query = true, a.dom = A.dom.data(), a.uid = nullptr; }, MAMDR_EINVAL, null_pq, false);
    refuse(TOPK_FORM, "per query, null domain", [](Args& a) { a.per_query = true, a.dom = nullptr; }, MAMDR_EINVAL, null_pq, false);
    refuse(TOPK_FORM, "per query, null ids_out", [](Args& a) { a.per_query = true, a.dom = A.dom.data(), a.ids_out = nullptr; }, MAMDR_EINVAL, null_pq, false);
    refuse(TOPK_FORM, "uid + 2", [](Args& a) { a.uid = shifted(a.uid, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "domain + 2", [](Args& a) { a.per_query = true, a.dom = shifted(A.dom.data(), 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "cand + 2", [](Args& a) { a.cand = shifted(a.cand, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "excl_ids + 2", [](Args& a) { a.excl_ids = shifted(a.excl_ids, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "ids_out + 2", [](Args& a) { a.ids_out = shifted(a.ids_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "scores_out + 2", [](Args& a) { a.scores_out = shifted(a.scores_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "scores_all + 2", [](Args& a) { a.scores_all = shifted(a.scores_all, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "excl_off + 4", [](Args& a) { a.excl_off = shifted(a.excl_off, 4); }, MAMDR_EINVAL, unaligned, false);
    refuse(TOPK_FORM, "exclusion offsets alone", [](Args& a) { a.excl_ids = nullptr; }, MAMDR_EINVAL, excl, false);
    refuse(TOPK_FORM, "exclusion ids alone", [](Args& a) { a.excl_off = nullptr; }, MAMDR_EINVAL, excl, false);
    refuse(TOPK_FORM, "k 0", [](Args& a) { a.k = 0; }, MAMDR_EINVAL, text("%s: k %d outside [1, %d]", "fn", 0, 128), false);
    refuse(TOPK_FORM, "k 129", [](Args& a) { a.k = 129; }, MAMDR_EINVAL, text("%s: k %d outside [1, %d]", "fn", 129, 128), false);
    refuse(TOPK_FORM, "n_query 0", [](Args& a) { a.n_query = 0; }, MAMDR_EINVAL, text("%s: n_query %d must be positive", "fn", 0), false);
    refuse(TOPK_FORM, "n_cand 0", [](Args& a) { a.n_cand = 0; }, MAMDR_EINVAL, text("%s: n_cand %lld with a candidate list given", "fn", 0LL), false);
    refuse(TOPK_FORM, "domain -1", [](Args& a) { a.domain = -1; }, MAMDR_EINVAL, text("%s: domain %d outside [0, %d)", "fn", -1, 3), false);
    refuse(TOPK_FORM, "domain n_domain", [](Args& a) { a.domain = 3; }, MAMDR_EINVAL, text("%s: domain %d outside [0, %d)", "fn", 3, 3), false);
    // the order of the checks decides what a doubly wrong call reports: the domain, then the contract, then the state
    refuse(TOPK_FORM, "domain 3 and n_query 0", [](Args& a) { a.domain = 3, a.n_query = 0; }, MAMDR_EINVAL, text("%s: domain %d outside [0, %d)", "fn", 3, 3), false);
    refuse(TOPK_FORM, "n_query 0 and k 0", [](Args& a) { a.n_query = 0, a.k = 0; }, MAMDR_EINVAL, text("%s: n_query %d must be positive", "fn", 0), false);
    refuse(TOPK_FORM, "k 0, not ready", [](Args& a) { a.k = 0, a.is_ready = false; }, MAMDR_EINVAL, text("%s: k %d outside [1, %d]", "fn", 0, 128), false);
    refuse(TOPK_FORM, "not ready", [](Args& a) { a.is_ready = false; }, MAMDR_ESTATE, "state incomplete", false);
    // ---- ranks
    const std::string null_rank = "fn: null uid / target offsets / rank / live output pointer";
    refuse(RANK_FORM, "null uid", [](Args& a) { a.uid = nullptr; }, MAMDR_EINVAL, null_rank, false);
    refuse(RANK_FORM, "null target offsets", [](Args& a) { a.list_off = nullptr; }, MAMDR_EINVAL, null_rank, false);
    refuse(RANK_FORM, "null rank_out", [](Args& a) { a.rank_out = nullptr; }, MAMDR_EINVAL, null_rank, false);
    refuse(RANK_FORM, "null live_out", [](Args& a) { a.live_out = nullptr; }, MAMDR_EINVAL, null_rank, false);
    refuse(RANK_FORM, "uid + 2", [](Args& a) { a.uid = shifted(a.uid, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "cand + 2", [](Args& a) { a.cand = shifted(a.cand, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "excl_ids + 2", [](Args& a) { a.excl_ids = shifted(a.excl_ids, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "tgt_ids + 2", [](Args& a) { a.list_ids = shifted(a.list_ids, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "rank_out + 2", [](Args& a) { a.rank_out = shifted(a.rank_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "score_out + 2", [](Args& a) { a.score_out = shifted(a.score_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "live_out + 2", [](Args& a) { a.live_out = shifted(a.live_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "excl_off + 4", [](Args& a) { a.excl_off = shifted(a.excl_off, 4); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "tgt_off + 4", [](Args& a) { a.list_off = shifted(a.list_off, 4); }, MAMDR_EINVAL, unaligned, false);
    refuse(RANK_FORM, "exclusion offsets alone", [](Args& a) { a.excl_ids = nullptr; }, MAMDR_EINVAL, excl, false);
    refuse(RANK_FORM, "exclusion ids alone", [](Args& a) { a.excl_off = nullptr; }, MAMDR_EINVAL, excl, false);
    refuse(RANK_FORM, "n_query 0", [](Args& a) { a.n_query = 0; }, MAMDR_EINVAL, text("%s: n_query %d must be positive", "fn", 0), false);
    refuse(RANK_FORM, "n_cand 0", [](Args& a) { a.n_cand = 0; }, MAMDR_EINVAL, text("%s: n_cand %lld with a candidate list given", "fn", 0LL), false);
    refuse(RANK_FORM, "domain -1", [](Args& a) { a.domain = -1; }, MAMDR_EINVAL, text("%s: domain %d outside [0, %d)", "fn", -1, 3), false);
    refuse(RANK_FORM, "domain n_domain", [](Args& a) { a.domain = 3; }, MAMDR_EINVAL, text("%s: domain %d outside [0, %d)", "fn", 3, 3), false);
    refuse(RANK_FORM, "not ready", [](Args& a) { a.is_ready = false; }, MAMDR_ESTATE, "state incomplete", false);
    refuse(RANK_FORM, "offsets start at 1", [](Args& a) { for (int64_t& o : a.off) o += 1; }, MAMDR_EINVAL,
           text("%s: the %s offsets start at %lld, not 0", "fn", "target", 1LL), true);
    refuse(RANK_FORM, "offsets descend at query 3", [](Args& a) { a.off[4] = a.off[3] - 1; }, MAMDR_EINVAL,
           text("%s: the %s offsets descend at query %d", "fn", "target", 3), true);
    refuse(RANK_FORM, "targets without ids", [](Args& a) { a.list_ids = nullptr; }, MAMDR_EINVAL,
           text("%s: %lld targets without their ids", "fn", 10LL), true);
    // ---- slates
    const std::string null_slates = "fn: null uid / slate offsets / position output pointer";
    refuse(SLATES_FORM, "null uid", [](Args& a) { a.uid = nullptr; }, MAMDR_EINVAL, null_slates, false);
    refuse(SLATES_FORM, "null slate offsets", [](Args& a) { a.list_off = nullptr; }, MAMDR_EINVAL, null_slates, false);
    refuse(SLATES_FORM, "null pos_out", [](Args& a) { a.pos_out = nullptr; }, MAMDR_EINVAL, null_slates, false);
    refuse(SLATES_FORM, "uid + 2", [](Args& a) { a.uid = shifted(a.uid, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(SLATES_FORM, "slate_ids + 2", [](Args& a) { a.list_ids = shifted(a.list_ids, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(SLATES_FORM, "score_out + 2", [](Args& a) { a.score_out = shifted(a.score_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(SLATES_FORM, "pos_out + 2", [](Args& a) { a.pos_out = shifted(a.pos_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(SLATES_FORM, "order_out + 2", [](Args& a) { a.order_out = shifted(a.order_out, 2); }, MAMDR_EINVAL, unaligned, false);
    refuse(SLATES_FORM, "slate_off + 4", [](Args& a) { a.list_off = shifted(a.list_off, 4); }, MAMDR_EINVAL, unaligned, false);
    refuse(SLATES_FORM, "n_query 0", [](Args& a) { a.n_query = 0; }, MAMDR_EINVAL, text("%s: n_query %d must be positive", "fn", 0), false);
    refuse(SLATES_FORM, "domain -1", [](Args& a) { a.domain = -1; }, MAMDR_EINVAL, text("%s: domain %d outside [0, %d)", "fn", -1, 3), false);
    refuse(SLATES_FORM, "domain n_domain", [](Args& a) { a.domain = 3; }, MAMDR_EINVAL, text("%s: domain %d outside [0, %d)", "fn", 3, 3), false);
    refuse(SLATES_FORM, "not ready", [](Args& a) { a.is_ready = false; }, MAMDR_ESTATE, "state incomplete", false);
    refuse(SLATES_FORM, "offsets start at 1", [](Args& a) { for (int64_t& o : a.off) o += 1; }, MAMDR_EINVAL,
           text("%s: the %s offsets start at %lld, not 0", "fn", "slate", 1LL), true);
    refuse(SLATES_FORM, "offsets descend at query 3", [](Args& a) { a.off[4] = a.off[3] - 1; }, MAMDR_EINVAL,
           text("%s: the %s offsets descend at query %d", "fn", "slate", 3), true);
    refuse(SLATES_FORM, "a slate of 2^31 entries", [](Args& a) { for (size_t q = 3; q < a.off.size(); ++q) a.off[q] += (1LL << 31) - 3; },
           MAMDR_EINVAL, text("%s: slate %d has %lld entries: positions are int32", "fn", 2, 1LL << 31), true);
    refuse(SLATES_FORM, "entries without ids", [](Args& a) { a.list_ids = nullptr; }, MAMDR_EINVAL,
           text("%s: %lld entries without their ids", "fn", 10LL), true);
}

int main() {
    long walks = 0;
    for (const int32_t n_query : N_QUERY)
        for (const int chunk : REC_CHUNKS) {
            for (const int64_t n_cand : cand_counts(chunk)) {
                walks += walk_topk(n_query, chunk, n_cand, false, true);
                walks += walk_topk(n_query, chunk, n_cand, true, true);
                walks += walk_topk(n_query, chunk, n_cand, false, false);       // no list: the catalogue
                for (int pattern = 0; pattern < 5; ++pattern) walks += walk_rank(n_query, chunk, n_cand, pattern);
            }
        }
    for (const int32_t n_query : N_QUERY)
        for (int pattern = 0; pattern < 5; ++pattern) {
            walks += walk_slates(n_query, pattern, true);
            walks += walk_slates(n_query, pattern, false);
        }
    refusals();
    std::printf("%ld calls walked, %ld refusals, %ld checks, %d failures\n", walks, rows, checks, fails);
    return fails ? 1 : 0;
}
