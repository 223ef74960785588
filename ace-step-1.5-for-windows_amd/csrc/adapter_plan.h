// adapter_plan.h - the adapter merge (ace355_dit_set_adapters / _mixed / _dora) as data, in the shape of attn_plan.h: what a call asks for
// (AdapterCall: the three term arrays of the ABI, the shape of every target they name, the targets applied now) and what
// set_adapters_impl then does (AdapterPlan: the targets in launch order, the device table, the two scratch sizes, the launch list).
// plan_adapters is a pure function of the call: no HIP call, no global, no environment, and device pointers only as numbers (null tests,
// and 16-byte alignment of w2), so ace355_adapter_plan can answer for any call on a machine without a GPU.  The structs the merge
// kernels read (lora.hip, lokr.hip, dora.hip) live here too; the header compiles with a plain host compiler.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/ace355.h"

#if defined(__HIPCC__)
#define ACE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ACE_HD inline
#endif

namespace ace355 {

typedef uint16_t bf16_t;  // raw bf16 bits

// ------------------------------------------------------------------ what the kernels read
// LoRA merge (lora.hip): one launch over the tiles of every target weight the call rewrites
constexpr int LORA_TILE_ROWS = 64, LORA_TILE_COLS = 128;
struct LoraTermDev {
    const bf16_t* A;   // lora_A.weight [rank, cols]
    const bf16_t* B;   // lora_B.weight [rows, rank]
    int rank;
    float scale;
};
struct LoraTargetDev {
    bf16_t* dst;         // live packed buffer
    const bf16_t* src;   // its pristine copy (same layout)
    long ld;             // packed row pitch (= cols)
    long row0;           // pack_row arguments of the target
    int mode, p0;
    int rows, cols;      // reference shape [out, in]; cols % 8 == 0
    int tile0, tiles_n;  // first tile of this target in the launch, column tiles per row tile
    int term0, nterms;   // terms [term0, term0 + nterms) of the term table; 0: copy the pristine rows back
};
// DoRA (dora.h, dora.hip): W' = bf16_rne(V f), V the fp32 value the plain merge would round and f = 1 + m (g / (||V|| + eps) - 1) per
// row (per_input 0) or per column (per_input 1).  A DoRA target's tiles run twice through its merge kernel (`pass` 1: fp64 partial sums
// of squares into `part`; `pass` 2: V f), launch_dora_factors in between forms f.  One DoraDev per target of a DoRA launch, at the
// target's index.
struct DoraDev {
    double* part;        // per_input 0: [tiles_n][rows], per_input 1: [tiles_m][cols] (scratch of the handle)
    float* f;            // [n]
    const float* g;      // [n]: dora_scale / lora_magnitude_vector in reference order
    int per_input;
    int n, ntiles;       // rows and column tiles per row, or columns and row tiles per column
    float eps, m;
};
// LoKr merge (lokr.hip): W' = bf16_rne(float(W0) + sum_j s_j (W1_j kron W2_j)).  A pre-pass writes the fp32 product a @ b of every
// decomposed factor into a scratch table of the handle; one merge launch then covers the tiles of every Kronecker target
// (LoraTargetDev, as the LoRA merge: nterms 0 copies the pristine rows back).
constexpr int LOKR_TILE_ROWS = 64, LOKR_TILE_COLS = 128;
constexpr int LOKR_FACTOR_ROWS = 64, LOKR_FACTOR_COLS = 128;   // factor pre-pass tile
static_assert(LORA_TILE_ROWS == LOKR_TILE_ROWS && LORA_TILE_COLS == LOKR_TILE_COLS, "dora.h: one tile shape for both merge kernels");
// LDS floats of the merge kernel: the W1 and W2 sub-blocks of one (tile, term).  With a = min(out_k, 64), b = min(in_n, 128) a tile
// meets at most (63 / a + 2)(127 / b + 2) entries of W1 (exactly 64 / a resp. 128 / b where a | 64 resp. b | 128, tiles being aligned)
// and a x b of W2 (row pitch lokr_w2_pitch(b)): the sum peaks at a = b = 1 (a dense W1) with 64 x 128 + 1 and at a = 64, b = 128 with
// 4 + 64 x 132.  A launch asks for the largest need among its terms (lokr_lds_floats), so the usual splits leave room for more
// workgroups per CU.
constexpr int LOKR_LDS_FLOATS = 64 * 132 + 64;
// LDS row pitch of a staged W2 block of nn columns: a multiple of 4 floats where the 16-byte paths need it, odd otherwise
ACE_HD int lokr_w2_pitch(int nn) { return nn % 4 == 0 ? nn + 4 : nn | 1; }
// worst case over the tiles of a term (<= LOKR_LDS_FLOATS for every split)
inline int lokr_lds_floats(int out_k, int in_n) {
    constexpr int TM = LOKR_TILE_ROWS, TN = LOKR_TILE_COLS;
    const int a = out_k < TM ? out_k : TM, b = in_n < TN ? in_n : TN;
    const int nl = TM % a == 0 && out_k <= TM ? TM / a : (TM - 1) / a + 2, nm = TN % b == 0 && in_n <= TN ? TN / b : (TN - 1) / b + 2;
    return ((nl * nm + 3) & ~3) + a * lokr_w2_pitch(b);
}
struct KronFactorDev {   // one decomposed factor: dst [rows, cols] fp32 = a [rows, rank] @ b [rank, cols]
    const bf16_t* a;
    const bf16_t* b;
    float* dst;
    int rows, cols, rank;
    int tile0, tiles_n;  // first tile of this factor in the pre-pass launch, column tiles per row tile
};
struct KronTermDev {
    const void* w1;      // [out_l, in_m]: bf16 as given (w1_f32 0) or the fp32 product in the scratch table (w1_f32 1)
    const void* w2;      // [out_k, in_n], likewise
    int w1_f32, w2_f32;
    int out_l, out_k, in_m, in_n;
    float scale;
    int wide;            // in_n % 8 == 0, in_n <= LOKR_TILE_COLS and w2 16-byte aligned: W2 is staged and read 16 bytes at a time
};

// ------------------------------------------------------------------ the projections of a decoder layer
// The eleven adapter target kinds of a layer, "layers.{i}.<name>", and their reference shapes [out, in]: the one place the projection
// shapes follow from the configuration (dit.hip packs by it, ace355_adapter_plan answers by it)
enum ProjKind { PROJ_SELF_Q, PROJ_SELF_K, PROJ_SELF_V, PROJ_SELF_O, PROJ_CROSS_Q, PROJ_CROSS_K, PROJ_CROSS_V, PROJ_CROSS_O, PROJ_GATE,
                PROJ_UP, PROJ_DOWN, PROJ_KINDS };
inline int proj_kind(const std::string& rest) {
    static const char* const names[PROJ_KINDS] = {
        "self_attn.q_proj.weight", "self_attn.k_proj.weight", "self_attn.v_proj.weight", "self_attn.o_proj.weight",
        "cross_attn.q_proj.weight", "cross_attn.k_proj.weight", "cross_attn.v_proj.weight", "cross_attn.o_proj.weight",
        "mlp.gate_proj.weight", "mlp.up_proj.weight", "mlp.down_proj.weight"};
    for (int k = 0; k < PROJ_KINDS; ++k) if (rest == names[k]) return k;
    return -1;
}
struct ProjShape { long rows, cols; };
inline ProjShape proj_shape(const ace355_dit_config& c, int kind) {
    const long D = c.hidden_size, F = c.intermediate_size, QD = (long)c.num_heads * 128, KVD = (long)c.num_kv_heads * 128;
    switch (kind) {
    case PROJ_SELF_Q: case PROJ_CROSS_Q: return {QD, D};
    case PROJ_SELF_K: case PROJ_SELF_V: case PROJ_CROSS_K: case PROJ_CROSS_V: return {KVD, D};
    case PROJ_SELF_O: case PROJ_CROSS_O: return {D, QD};
    case PROJ_GATE: case PROJ_UP: return {F, D};
    default: return {D, F};
    }
}

// ------------------------------------------------------------------ the call
// A name of the call, resolved by the caller: id < 0 = not a target; else one id per target (layer x PROJ_KINDS + kind) and its shape
constexpr int ADAPTER_CROSS_KV = 1, ADAPTER_CROSS_O = 2;
struct AdapterRef {
    const char* name;
    int id;
    long rows, cols;
    int cross;   // ADAPTER_CROSS_*: a cross-attention k / v resp. o projection (condition slots built from it go stale), else 0
};
inline AdapterRef adapter_ref(const ace355_dit_config& c, const char* name, int layer, int kind) {
    const ProjShape p = proj_shape(c, kind);
    return {name, layer * PROJ_KINDS + kind, p.rows, p.cols,
            kind == PROJ_CROSS_K || kind == PROJ_CROSS_V ? ADAPTER_CROSS_KV : kind == PROJ_CROSS_O ? ADAPTER_CROSS_O : 0};
}
// `name` as a target of a decoder with configuration c, id -1 where it is none (dit.hip: the layer-key parser lives with the loaders)
AdapterRef adapter_ref_of(const ace355_dit_config& c, const char* name);

struct AdapterCall {
    const ace355_lora_term* lora; int n_lora;
    const ace355_kron_term* kron; int n_kron;
    const ace355_dora_term* dora; int n_dora;
    const AdapterRef *lora_ref, *kron_ref, *dora_ref;   // one per term (read only where the term array itself passes its checks)
    const AdapterRef* applied; int n_applied;           // the targets whose live rows hold a merge now (all valid, each once)
};

// ------------------------------------------------------------------ the plan
// Which launches a target rides: by the kernel that forms its V, plain or (a live DoRA term) in the two-pass launches.  A restored
// target (no term now) rides with the Kronecker launch when the call has a live Kronecker term and with the LoRA launch otherwise.
enum AdapterClass { ADAPTER_LORA, ADAPTER_KRON, ADAPTER_DORA_LORA, ADAPTER_DORA_KRON, ADAPTER_CLASSES };
// The device table: every section starts 256-byte aligned, an empty one has 0 bytes
enum AdapterSection { SEC_LORA_TARGETS, SEC_LORA_TERMS, SEC_KRON_TARGETS, SEC_KRON_TERMS, SEC_KRON_FACTORS, SEC_DORA_LORA_TARGETS,
                      SEC_DORA_LORA_ROWS, SEC_DORA_KRON_TARGETS, SEC_DORA_KRON_ROWS, ADAPTER_SECTIONS };
constexpr int ADAPTER_TARGET_SECTION[ADAPTER_CLASSES] = {SEC_LORA_TARGETS, SEC_KRON_TARGETS, SEC_DORA_LORA_TARGETS, SEC_DORA_KRON_TARGETS};
enum AdapterKernel { ADAPTER_KERNEL_LORA_MERGE, ADAPTER_KERNEL_KRON_FACTORS, ADAPTER_KERNEL_KRON_MERGE, ADAPTER_KERNEL_DORA_FACTORS };

struct AdapterTarget {
    const char* name;    // the caller's string
    int cls;             // AdapterClass
    int row;             // its LoraTargetDev is row `row` of section ADAPTER_TARGET_SECTION[cls]; its DoraDev, if any, row `row` of the next
    int rows, cols;
    int tile0, tiles_n;  // tiles [tile0, tile0 + ceil(rows / 64) tiles_n) of its class's launches
    int term0, nterms;   // rows of SEC_LORA_TERMS resp. SEC_KRON_TERMS; 0 terms: the pristine rows (rescaled, in a DoRA class)
    bool restored;
};
struct AdapterLaunch {
    int kernel, pass;    // AdapterKernel; pass 0 plain, 1 / 2 the DoRA passes of a merge kernel
    int n;               // entries of its first section
    int grid_x, grid_y;  // 256 threads each
    int lds_bytes;       // dynamic LDS
    int sec[3];          // the sections it reads (-1: none): merges {targets, terms, DoRA rows}, the factor kernels {their rows}
};
struct AdapterPlan {
    int code = ACE355_OK;
    std::string error;                    // code != 0: the message, and nothing below is set
    std::vector<AdapterTarget> targets;   // merged targets in first-mention order, then the restored ones; empty: the call does nothing
    int n_merged = 0;
    size_t at[ADAPTER_SECTIONS] = {}, bytes[ADAPTER_SECTIONS] = {};
    std::vector<char> table;              // the table's image.  Pointers into the handle's buffers are held as byte offsets (factor
                                          // products in kscratch, DoRA partials and factors in dscratch) resp. null (a target's packed
                                          // rows) until adapter_table_patch
    size_t kscratch_floats = 0, dscratch_bytes = 0;
    std::vector<AdapterLaunch> launches;  // in stream order
    bool stale_kv = false, stale_o = false;
};

namespace adapter_detail {
template <typename T> inline T row_at(const AdapterPlan& p, int sec, size_t i) {
    T v;
    memcpy(&v, p.table.data() + p.at[sec] + i * sizeof(T), sizeof(T));
    return v;
}
template <typename T> inline void row_put(AdapterPlan& p, int sec, size_t i, const T& v) {
    memcpy(p.table.data() + p.at[sec] + i * sizeof(T), &v, sizeof(T));
}
template <typename P> inline P based(uintptr_t base, P offset) { return (P)(base + (uintptr_t)offset); }
inline AdapterPlan refuse(const std::string& msg) {
    AdapterPlan p;
    p.code = ACE355_ERR_INVALID;
    p.error = msg;
    return p;
}
inline AdapterPlan invalid(const char* msg) { return refuse(std::string("invalid argument: ") + msg); }
inline AdapterPlan not_a_target(const char* name) {
    return refuse(std::string("set_adapters: '") + name + "' is not a LoRA target (layers.{i}.{self_attn,cross_attn}.{q,k,v,o}_proj.weight, "
                  "layers.{i}.mlp.{gate,up,down}_proj.weight)");
}
}  // namespace adapter_detail

// What is wrong with the three term arrays themselves, null: nothing.  (set_adapters_impl asks before it resolves the names.)
inline const char* adapter_arrays_error(const AdapterCall& c) {
    if (!(c.n_lora >= 0 && (c.n_lora == 0 || c.lora))) return "set_adapters: terms";
    if (!(c.n_kron >= 0 && (c.n_kron == 0 || c.kron))) return "set_adapters: kron terms";
    if (!(c.n_dora >= 0 && (c.n_dora == 0 || c.dora))) return "set_adapters: dora terms";
    return nullptr;
}

inline AdapterPlan plan_adapters(const AdapterCall& c) {
    using namespace adapter_detail;
    if (const char* m = adapter_arrays_error(c)) return invalid(m);
    // the terms per target, in call order; scale 0 drops a term
    struct Group { AdapterRef ref; std::vector<int> lora, kron; int dora; };
    std::vector<Group> order;
    int ids = 0;
    for (int i = 0; i < c.n_lora; ++i) ids = std::max(ids, c.lora_ref[i].id + 1);
    for (int i = 0; i < c.n_kron; ++i) ids = std::max(ids, c.kron_ref[i].id + 1);
    for (int i = 0; i < c.n_dora; ++i) ids = std::max(ids, c.dora_ref[i].id + 1);
    for (int i = 0; i < c.n_applied; ++i) ids = std::max(ids, c.applied[i].id + 1);
    std::vector<int> slot(ids, -1);           // id -> index in `order`
    enum { BY_LORA = 1, BY_ADDITIVE = 2, BY_DORA = 4 };
    std::vector<unsigned char> named(ids, 0); // id -> which families name it, dropped terms included
    auto group_of = [&](const AdapterRef& r) -> Group& {
        if (slot[r.id] < 0) { slot[r.id] = (int)order.size(); order.push_back(Group{r, {}, {}, -1}); }
        return order[slot[r.id]];
    };
    for (int i = 0; i < c.n_lora; ++i) {
        const ace355_lora_term& t = c.lora[i];
        const AdapterRef& r = c.lora_ref[i];
        if (!(t.name && t.A_dev && t.B_dev)) return invalid("set_adapters: null name / A / B");
        if (r.id < 0) return not_a_target(t.name);
        if (!(t.rank >= 1 && std::isfinite(t.scale))) return invalid("set_adapters: rank must be >= 1 and scale finite");
        named[r.id] |= BY_LORA | BY_ADDITIVE;
        if (t.scale != 0.f) group_of(r).lora.push_back(i);
    }
    for (int i = 0; i < c.n_kron; ++i) {
        const ace355_kron_term& t = c.kron[i];
        const AdapterRef& r = c.kron_ref[i];
        if (!t.name) return invalid("set_adapters: null name in a Kronecker term");
        if (r.id < 0) return not_a_target(t.name);
        // exactly one of {w} / {w_a, w_b} per factor; r = 0 for a full factor, >= 1 for a decomposed one
        const bool f1 = t.w1_dev && !t.w1a_dev && !t.w1b_dev && t.r1 == 0, d1 = !t.w1_dev && t.w1a_dev && t.w1b_dev && t.r1 >= 1;
        const bool f2 = t.w2_dev && !t.w2a_dev && !t.w2b_dev && t.r2 == 0, d2 = !t.w2_dev && t.w2a_dev && t.w2b_dev && t.r2 >= 1;
        if (!(t.r1 >= 0 && t.r2 >= 0)) return invalid("set_adapters: a Kronecker factor's rank must be >= 0");
        if (!((f1 || d1) && (f2 || d2))) return invalid("set_adapters: each Kronecker factor needs exactly one of {w} (rank 0) / {w_a, w_b} (rank >= 1)");
        if (!(t.out_l >= 1 && t.out_k >= 1 && t.in_m >= 1 && t.in_n >= 1 && (long)t.out_l * t.out_k == r.rows && (long)t.in_m * t.in_n == r.cols))
            return invalid("set_adapters: out_l x out_k / in_m x in_n do not give the target's [out, in]");
        if (!std::isfinite(t.scale)) return invalid("set_adapters: scale must be finite");
        if (!(lokr_lds_floats(t.out_k, t.in_n) <= LOKR_LDS_FLOATS)) return invalid("set_adapters: Kronecker split exceeds the merge tile's LDS");
        if (named[r.id] & BY_LORA)   // the reference never has both (H/lora/lifecycle.py:244-246)
            return refuse(std::string("set_adapters: '") + t.name + "' is named by a LoRA term and by a Kronecker term");
        named[r.id] |= BY_ADDITIVE;
        if (t.scale != 0.f) group_of(r).kron.push_back(i);
    }
    for (int i = 0; i < c.n_dora; ++i) {
        const ace355_dora_term& t = c.dora[i];
        const AdapterRef& r = c.dora_ref[i];
        if (!(t.name && t.g_dev)) return invalid("set_adapters: null name / g in a DoRA term");
        if (r.id < 0) return not_a_target(t.name);
        if (!(t.per_input == 0 || t.per_input == 1)) return invalid("set_adapters: a DoRA term's per_input must be 0 or 1");
        if (!(std::isfinite(t.eps) && t.eps >= 0.f && std::isfinite(t.multiplier)))
            return invalid("set_adapters: a DoRA term's eps must be finite and >= 0 and its multiplier finite");
        if (named[r.id] & BY_DORA) return refuse(std::string("set_adapters: two DoRA terms name '") + t.name + "'");
        named[r.id] |= BY_DORA;
        if (t.multiplier == 0.f) continue;   // f = 1
        if (!(named[r.id] & BY_ADDITIVE))
            return refuse(std::string("set_adapters: the DoRA term on '") + t.name + "' has no LoRA / Kronecker term beside it in this call");
        group_of(r).dora = i;   // (every additive term of the target at scale 0: V = W0, still rescaled)
    }
    AdapterPlan p;
    p.n_merged = (int)order.size();
    for (int i = 0; i < c.n_applied; ++i)   // merged before, no term now: its rows go back to the base
        if (slot[c.applied[i].id] < 0) group_of(c.applied[i]);
    if (order.empty()) return p;
    bool any_kron = false;
    for (const Group& g : order) any_kron = any_kron || !g.kron.empty();

    // the rows of every section, the scratch regions (each carved once, its offset in the row that points at it) and the tile ranges
    std::vector<LoraTargetDev> tg[ADAPTER_CLASSES];
    std::vector<DoraDev> dv[ADAPTER_CLASSES];   // (the two DoRA classes)
    std::vector<LoraTermDev> tm;
    std::vector<KronTermDev> ktm;
    std::vector<KronFactorDev> jobs;
    int tiles[ADAPTER_CLASSES] = {}, jtiles = 0, klds = 4, dmax_n = 0;
    auto up16 = [](size_t b) { return (b + 15) / 16 * 16; };
    auto factor = [&](const void* a, const void* b, int rows, int cols, int rank) -> const void* {   // the fp32 product of a decomposed factor
        KronFactorDev f{};
        f.a = (const bf16_t*)a; f.b = (const bf16_t*)b; f.dst = (float*)(uintptr_t)(p.kscratch_floats * sizeof(float));
        f.rows = rows; f.cols = cols; f.rank = rank;
        f.tiles_n = (cols + LOKR_FACTOR_COLS - 1) / LOKR_FACTOR_COLS; f.tile0 = jtiles;
        jtiles += (rows + LOKR_FACTOR_ROWS - 1) / LOKR_FACTOR_ROWS * f.tiles_n;
        p.kscratch_floats += ((size_t)rows * cols + 3) / 4 * 4;
        jobs.push_back(f);
        return f.dst;
    };
    for (const Group& g : order) {
        const AdapterRef& r = g.ref;
        if (r.cols % 8 != 0) return invalid("set_adapters: target columns must be a multiple of 8");
        const bool to_kron = !g.kron.empty() || (g.lora.empty() && any_kron);
        const int cls = g.dora >= 0 ? (to_kron ? ADAPTER_DORA_KRON : ADAPTER_DORA_LORA) : (to_kron ? ADAPTER_KRON : ADAPTER_LORA);
        LoraTargetDev x{};
        x.rows = (int)r.rows; x.cols = (int)r.cols;
        x.tiles_n = (x.cols + LORA_TILE_COLS - 1) / LORA_TILE_COLS;
        x.tile0 = tiles[cls];
        tiles[cls] += (x.rows + LORA_TILE_ROWS - 1) / LORA_TILE_ROWS * x.tiles_n;
        if (g.dora >= 0) {   // per target its fp64 partials, then its fp32 factors
            const ace355_dora_term& t = c.dora[g.dora];
            DoraDev v{};
            v.per_input = t.per_input; v.eps = t.eps; v.m = t.multiplier; v.g = t.g_dev;
            v.n = t.per_input ? x.cols : x.rows;
            v.ntiles = t.per_input ? (x.rows + LORA_TILE_ROWS - 1) / LORA_TILE_ROWS : x.tiles_n;
            v.part = (double*)(uintptr_t)p.dscratch_bytes;
            p.dscratch_bytes += up16((size_t)v.n * v.ntiles * sizeof(double));
            v.f = (float*)(uintptr_t)p.dscratch_bytes;
            p.dscratch_bytes += up16((size_t)v.n * sizeof(float));
            dmax_n = std::max(dmax_n, v.n);
            dv[cls].push_back(v);
        }
        if (to_kron) {
            x.term0 = (int)ktm.size();
            for (int i : g.kron) {
                const ace355_kron_term& t = c.kron[i];
                KronTermDev u{};
                u.w1 = t.r1 ? factor(t.w1a_dev, t.w1b_dev, t.out_l, t.in_m, t.r1) : t.w1_dev; u.w1_f32 = t.r1 ? 1 : 0;
                u.w2 = t.r2 ? factor(t.w2a_dev, t.w2b_dev, t.out_k, t.in_n, t.r2) : t.w2_dev; u.w2_f32 = t.r2 ? 1 : 0;
                u.out_l = t.out_l; u.out_k = t.out_k; u.in_m = t.in_m; u.in_n = t.in_n; u.scale = t.scale;
                // (a product's region starts a multiple of 4 floats into the scratch, itself 16-byte aligned)
                u.wide = t.in_n % 8 == 0 && t.in_n <= LOKR_TILE_COLS && (u.w2_f32 || (uintptr_t)u.w2 % 16 == 0);
                klds = std::max(klds, lokr_lds_floats(t.out_k, t.in_n));
                ktm.push_back(u);
            }
            x.nterms = (int)ktm.size() - x.term0;
        } else {
            x.term0 = (int)tm.size();
            for (int i : g.lora) tm.push_back(LoraTermDev{(const bf16_t*)c.lora[i].A_dev, (const bf16_t*)c.lora[i].B_dev, c.lora[i].rank, c.lora[i].scale});
            x.nterms = (int)tm.size() - x.term0;
        }
        p.targets.push_back(AdapterTarget{r.name, cls, (int)tg[cls].size(), x.rows, x.cols, x.tile0, x.tiles_n, x.term0, x.nterms,
                                          (int)p.targets.size() >= p.n_merged});
        tg[cls].push_back(x);
        p.stale_kv = p.stale_kv || r.cross == ADAPTER_CROSS_KV;
        p.stale_o = p.stale_o || r.cross == ADAPTER_CROSS_O;
    }

    // the table: one rule for every section
    const struct { const void* rows; size_t bytes; } src[ADAPTER_SECTIONS] = {
        {tg[ADAPTER_LORA].data(), tg[ADAPTER_LORA].size() * sizeof(LoraTargetDev)}, {tm.data(), tm.size() * sizeof(LoraTermDev)},
        {tg[ADAPTER_KRON].data(), tg[ADAPTER_KRON].size() * sizeof(LoraTargetDev)}, {ktm.data(), ktm.size() * sizeof(KronTermDev)},
        {jobs.data(), jobs.size() * sizeof(KronFactorDev)},
        {tg[ADAPTER_DORA_LORA].data(), tg[ADAPTER_DORA_LORA].size() * sizeof(LoraTargetDev)},
        {dv[ADAPTER_DORA_LORA].data(), dv[ADAPTER_DORA_LORA].size() * sizeof(DoraDev)},
        {tg[ADAPTER_DORA_KRON].data(), tg[ADAPTER_DORA_KRON].size() * sizeof(LoraTargetDev)},
        {dv[ADAPTER_DORA_KRON].data(), dv[ADAPTER_DORA_KRON].size() * sizeof(DoraDev)}};
    size_t end = 0;
    for (int s = 0; s < ADAPTER_SECTIONS; ++s) {
        p.at[s] = end; p.bytes[s] = src[s].bytes;
        end += (src[s].bytes + 255) / 256 * 256;
    }
    p.table.assign(end, 0);
    for (int s = 0; s < ADAPTER_SECTIONS; ++s)
        if (src[s].bytes) memcpy(p.table.data() + p.at[s], src[s].rows, src[s].bytes);

    // the launches, in stream order: the plain merges, then pass 1 of both kernels, the DoRA factors, pass 2 of both
    auto merge = [&](int kernel, int cls, int pass) {
        if (tg[cls].empty()) return;
        const bool kr = kernel == ADAPTER_KERNEL_KRON_MERGE;
        p.launches.push_back(AdapterLaunch{kernel, pass, (int)tg[cls].size(), tiles[cls], 1, kr ? klds * (int)sizeof(float) : 0,
                                           {ADAPTER_TARGET_SECTION[cls], kr ? SEC_KRON_TERMS : SEC_LORA_TERMS, pass ? ADAPTER_TARGET_SECTION[cls] + 1 : -1}});
    };
    auto dora_factors = [&](int cls) {
        if (dv[cls].empty()) return;
        p.launches.push_back(AdapterLaunch{ADAPTER_KERNEL_DORA_FACTORS, 0, (int)dv[cls].size(), (dmax_n + 255) / 256, (int)dv[cls].size(), 0,
                                           {ADAPTER_TARGET_SECTION[cls] + 1, -1, -1}});
    };
    merge(ADAPTER_KERNEL_LORA_MERGE, ADAPTER_LORA, 0);
    if (!jobs.empty()) p.launches.push_back(AdapterLaunch{ADAPTER_KERNEL_KRON_FACTORS, 0, (int)jobs.size(), jtiles, 1, 0, {SEC_KRON_FACTORS, -1, -1}});
    merge(ADAPTER_KERNEL_KRON_MERGE, ADAPTER_KRON, 0);
    merge(ADAPTER_KERNEL_LORA_MERGE, ADAPTER_DORA_LORA, 1);
    merge(ADAPTER_KERNEL_KRON_MERGE, ADAPTER_DORA_KRON, 1);
    dora_factors(ADAPTER_DORA_LORA);
    dora_factors(ADAPTER_DORA_KRON);
    merge(ADAPTER_KERNEL_LORA_MERGE, ADAPTER_DORA_LORA, 2);
    merge(ADAPTER_KERNEL_KRON_MERGE, ADAPTER_DORA_KRON, 2);
    return p;
}

// The handle's half of a target row: where its packed rows live
struct AdapterWhere {
    bf16_t* dst;
    const bf16_t* src;
    long ld, row0;
    int mode, p0;
};
// Turns the image into what the kernels read: where[i] goes into the row of targets[i], and every scratch offset gets its base.  Once.
inline void adapter_table_patch(AdapterPlan& p, const AdapterWhere* where, uintptr_t kscratch, uintptr_t dscratch) {
    using namespace adapter_detail;
    for (size_t i = 0; i < p.targets.size(); ++i) {
        const int sec = ADAPTER_TARGET_SECTION[p.targets[i].cls];
        LoraTargetDev x = row_at<LoraTargetDev>(p, sec, p.targets[i].row);
        x.dst = where[i].dst; x.src = where[i].src; x.ld = where[i].ld; x.row0 = where[i].row0; x.mode = where[i].mode; x.p0 = where[i].p0;
        row_put(p, sec, p.targets[i].row, x);
    }
    for (size_t i = 0; i < p.bytes[SEC_KRON_FACTORS] / sizeof(KronFactorDev); ++i) {
        KronFactorDev f = row_at<KronFactorDev>(p, SEC_KRON_FACTORS, i);
        f.dst = based(kscratch, f.dst);
        row_put(p, SEC_KRON_FACTORS, i, f);
    }
    for (size_t i = 0; i < p.bytes[SEC_KRON_TERMS] / sizeof(KronTermDev); ++i) {
        KronTermDev u = row_at<KronTermDev>(p, SEC_KRON_TERMS, i);
        if (u.w1_f32) u.w1 = based(kscratch, u.w1);
        if (u.w2_f32) u.w2 = based(kscratch, u.w2);
        row_put(p, SEC_KRON_TERMS, i, u);
    }
    for (int sec : {(int)SEC_DORA_LORA_ROWS, (int)SEC_DORA_KRON_ROWS})
        for (size_t i = 0; i < p.bytes[sec] / sizeof(DoraDev); ++i) {
            DoraDev v = row_at<DoraDev>(p, sec, i);
            v.part = based(dscratch, v.part); v.f = based(dscratch, v.f);
            row_put(p, sec, i, v);
        }
}

}  // namespace ace355
