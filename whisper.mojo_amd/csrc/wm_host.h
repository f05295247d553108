// wm_host.h — what every host source shares: the runtime's sources (whisper_mi.cpp and the subsystems behind wm_runtime.h, which
// includes this) and wm_ops.cpp (the wm_op_* test hooks), which needs no more than this.
// Internal to the library: everything declared here has hidden visibility, so none of it reaches the dynamic symbol table.
#pragma once
#include "../../include/whisper_mi.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <vector>

#include "wm_kernels.h"

#pragma GCC visibility push(hidden)

int fail(int code, const char* fmt, ...);  // sets wm_last_error, returns code
#define HIPCHK(expr)                                                                                     \
    do {                                                                                                 \
        hipError_t e_ = (expr);                                                                          \
        if (e_ != hipSuccess) return fail(WM_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)
#define WMCHK(expr)            \
    do {                       \
        int rc_ = (expr);      \
        if (rc_ != 0) return rc_; \
    } while (0)

// a launcher's status (wm_kernels.h WM_LAUNCH_*) as a C-ABI status: a refused shape is the caller's argument error
int launch_rc(int st);
#define LCHK(expr) WMCHK(launch_rc(expr))

#define DISPATCH_DT(dt, T, ...)              \
    do {                                     \
        if ((dt) == WM_F32) {                \
            typedef float T;                 \
            __VA_ARGS__;                     \
        } else if ((dt) == WM_BF16) {        \
            typedef wm::bf16 T;              \
            __VA_ARGS__;                     \
        } else {                             \
            typedef wm::f16 T;               \
            __VA_ARGS__;                     \
        }                                    \
    } while (0)

static inline size_t dt_size(int dt) { return dt == WM_F32 ? 4 : 2; }
static inline uint16_t f32_to_bf16_host(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);  // NaN stays NaN
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}
static inline uint16_t f32_to_f16_host(float f) {
    _Float16 h = (_Float16)f;
    uint16_t u;
    memcpy(&u, &h, 2);
    return u;
}

#pragma GCC visibility push(default)  // the types keep the visibility they always had; only the functions that lost `static` hide
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    int alloc(size_t n, bool zero = false) {
        release();  // re-allocation never leaks the previous block
        bytes = n ? n : 16;
        hipError_t e = hipMalloc(&p, bytes);
        if (e != hipSuccess) return fail(WM_E_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
        if (zero) {
            // hipMemset on device memory is asynchronous to the host and runs on the null stream, which the library's
            // non-blocking streams do not wait for: finish it here, or the first kernels on a fresh buffer can race the
            // zeroing (seen once in ~6 runs of the eight-slot test as a wrong token row)
            e = hipMemset(p, 0, bytes);
            if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
            if (e != hipSuccess) return fail(WM_E_HIP, "hipMemset: %s", hipGetErrorString(e));
        }
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    template <typename T> T* as() const { return (T*)p; }
};

// Scratch of one call, released on return.  Callers keep add()'s references for the whole call and call add() again later (in
// branches, in loops), so a buffer must never move: each lives in a node of its own, and no count has to be known ahead.
struct TmpDev {
    struct Node {
        DevBuf buf;
        Node* next;
    };
    Node* head = nullptr;
    ~TmpDev() {
        while (Node* n = head) {
            head = n->next;
            n->buf.release();
            delete n;
        }
    }
    DevBuf& add() {
        head = new Node{DevBuf(), head};
        return head->buf;
    }
};
#pragma GCC visibility pop

// host fp32 -> device buffer in dtype dt
int upload(DevBuf& b, const float* h, size_t n, int dt);
// the first n of n_dev elements from h, zeros behind them (n_dev <= n: no padding)
int upload_padded(DevBuf& b, const float* h, size_t n, size_t n_dev, int dt);
// rows of the 128-row panels that hold M rows: the tile kernels read whole panels of A
static inline size_t panel_rows(int M) { return ((size_t)M + 127) / 128 * 128; }
// n bytes as they are: ids, tables and control blocks
int upload_bytes(DevBuf& b, const void* h, size_t n);
// n device elements of dtype dt -> host fp32; the pitched form reads cols of every row of ld elements
int download_f32(float* dst, const DevBuf& b, size_t n, int dt);
int download_f32_rows(float* dst, const DevBuf& b, size_t rows, size_t cols, size_t ld, int dt);

static const float ATTN_SCALE = 1.0f / sqrtf(64.0f);  // every attention here has heads of 64 columns

#pragma GCC visibility push(default)
// One table of wm_set_sequence_bias: both lists validated, grouped by last id and copied to the device.  Immutable once
// built; the model, a held submit and a state's pending pass each hold a reference, so replacing the model's table changes none of them.
struct SeqTable {
    int gen = 0;  // the model's count of tables built: what a PassAsk carries and what pairs two submits
    int device = 0;  // where the buffers live: the last reference may drop while another device is current
    int n_seq = 0, n_slots = 0;
    DevBuf ids, off, bias, ban, slot_id, slot_off, slot_of;
    SeqTable() = default;
    SeqTable(const SeqTable&) = delete;
    SeqTable& operator=(const SeqTable&) = delete;
    ~SeqTable() {
        int cur = -1;
        const bool moved = hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
        for (DevBuf* b : {&ids, &off, &bias, &ban, &slot_id, &slot_off, &slot_of}) b->release();
        if (moved) (void)hipSetDevice(cur);
    }
    wm::SeqBiasCtl ctl(int eot) const {
        return wm::SeqBiasCtl{n_seq, n_slots, eot, ids.as<int>(), off.as<int>(), bias.as<float>(), ban.as<int>(), slot_id.as<int>(), slot_off.as<int>(), slot_of.as<int>()};
    }
};
// One table of wm_set_constraint: the phrases validated, their trie flattened to CSR and copied to the device.  Immutable
// and reference counted exactly as SeqTable is.  ids: the distinct ids of all phrases, ascending — what a pass's eot is checked against.
struct ConstraintTable {
    int gen = 0;     // the model's count of tables built: what pairs two submits
    int device = 0;  // where the buffers live
    int n_nodes = 0, dead = 0, n_phrases = 0, free_from = 0;
    std::vector<int32_t> ids;
    DevBuf edge_off, edge_id, edge_next, terminal;
    ConstraintTable() = default;
    ConstraintTable(const ConstraintTable&) = delete;
    ConstraintTable& operator=(const ConstraintTable&) = delete;
    ~ConstraintTable() {
        int cur = -1;
        const bool moved = hipGetDevice(&cur) == hipSuccess && cur != device && hipSetDevice(device) == hipSuccess;
        for (DevBuf* b : {&edge_off, &edge_id, &edge_next, &terminal}) b->release();
        if (moved) (void)hipSetDevice(cur);
    }
    bool holds(int id) const { return std::binary_search(ids.begin(), ids.end(), id); }
    wm::ConstraintCtl ctl(int eot) const {
        return wm::ConstraintCtl{n_nodes, dead, eot, free_from, edge_off.as<int>(), edge_id.as<int>(), edge_next.as<int>(), terminal.as<int>()};
    }
};
// What a sweep over the tied embedding reads: the final LayerNorm and the embedding in the decoder's operand dtype
struct VocabHead {
    const float *ln_g, *ln_b;
    const void* emb;
    int vocab, d_model;
};
#pragma GCC visibility pop

// the runtime's own wiring, which the hooks launch through (defined in whisper_mi.cpp, commented there)
int gemm_dispatch(int dt_in, int dt_out, const wm::GemmParams& p, int batch, hipStream_t st);
int ln_then_gemm(int dt_in, int dt_out, wm::GemmParams p, const float* x, const float* g, const float* b, hipStream_t st);
int dec_linear_dispatch(int dt, const wm::DecLinearParams& p, hipStream_t st);
int attn_decode_dispatch(int dt, const wm::AttnDecParams& p, hipStream_t st, const int* key_lo = nullptr, const int* utt_of = nullptr);
wm::DecLinearParams linear_block(const float* x, const float* ln_g, const float* ln_b, const void* W, const float* bias, int N, int K, int B,
                                 float* out, int ldo);
int ns_sweep(int T, const float* x, const VocabHead& h, int B, int npart, float* pmax, int* pidx, float* psum, int token, float* prob, float* lse,
             hipStream_t st);
int lang_list_check(int vocab, const int32_t* lang_ids, int n_lang);
int build_seq_table(std::shared_ptr<SeqTable>& out, int vocab, const int32_t* ids, const int32_t* off, const float* bias, int n_seq,
                    const int32_t* bad_ids, const int32_t* bad_off, int n_bad, std::vector<int32_t>* slot_ids = nullptr);
int build_constraint_table(std::shared_ptr<ConstraintTable>& out, int vocab, const int32_t* ids, const int32_t* off, int n_phrases, int free_from);
std::vector<float> conv_relayout(const float* w, int co, int ci, int cip);
// the vocabulary head of a hook (wm_ops.cpp): the K the logits kernels take, and x [B][K] fp32 + ln_g, ln_b + emb [N][K] in dtype on the device
int vocab_k_check(int K);
int upload_vocab_head(TmpDev& t, const float* x, const float* ln_g, const float* ln_b, const float* emb, int B, int N, int K, int dtype,
                      const float** dx, VocabHead* h);

#pragma GCC visibility pop
