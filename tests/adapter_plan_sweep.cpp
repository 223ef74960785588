// adapter_plan_sweep.cpp - plan_adapters (csrc/adapter_plan.h) as a stand-alone host program, for a build under AddressSanitizer and
// UBSan (tests/test_adapter_plan_cpu.py builds and runs it; it is never loaded into python and needs no GPU).
//   adapter_plan_sweep CALLS N
// CALLS lists calls with the names already resolved (test_adapter_plan_cpu.py writes it from tests/_adapter_plan_cases.py); each must
// end as the file says.  Then N seeded random calls, valid and invalid, on random configurations.  Every plan that is not a refusal is
// checked for the conditions the kernels rely on, and its table is filled the way set_adapters_impl does it, into buffers of exactly
// the plan's sizes, and every scratch region and table row it names is written through - an offset outside its buffer is a sanitizer report.
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>

#include "../ace-step-1.5-for-windows_amd/csrc/adapter_plan.h"

using namespace ace355;

#define REQUIRE(c)                                                              \
    do {                                                                        \
        if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); exit(1); }  \
    } while (0)

struct Call {
    std::vector<std::string> names;   // (stable storage: reserved before use)
    std::vector<ace355_lora_term> lora;
    std::vector<ace355_kron_term> kron;
    std::vector<ace355_dora_term> dora;
    std::vector<AdapterRef> lref, kref, dref, applied;
    AdapterCall call() const {
        return AdapterCall{lora.data(), (int)lora.size(), kron.data(), (int)kron.size(), dora.data(), (int)dora.size(),
                           lref.data(), kref.data(), dref.data(), applied.data(), (int)applied.size()};
    }
};

static const void* ptr(unsigned long long v) { return (const void*)(uintptr_t)v; }

// The conditions, then the fill.  Returns the plan's code.
static int run(const Call& c, AdapterPlan* out) {
    AdapterPlan p = plan_adapters(c.call());
    *out = p;
    if (p.code) { REQUIRE(p.code == ACE355_ERR_INVALID && !p.error.empty() && p.targets.empty() && p.table.empty()); return p.code; }
    if (p.targets.empty()) { REQUIRE(p.launches.empty() && p.table.empty() && !p.kscratch_floats && !p.dscratch_bytes); return 0; }
    size_t end = 0;
    for (int s = 0; s < ADAPTER_SECTIONS; ++s) {   // in order, aligned, disjoint, inside
        REQUIRE(p.at[s] % 256 == 0 && p.at[s] >= end && p.at[s] + p.bytes[s] <= p.table.size());
        end = p.at[s] + p.bytes[s];
    }
    int tiles[ADAPTER_CLASSES] = {}, count[ADAPTER_CLASSES] = {};
    for (const AdapterTarget& t : p.targets) {
        REQUIRE(t.cls >= 0 && t.cls < ADAPTER_CLASSES && t.row == count[t.cls] && t.tile0 == tiles[t.cls] && t.cols % 8 == 0);
        REQUIRE((size_t)(t.row + 1) * sizeof(LoraTargetDev) <= p.bytes[ADAPTER_TARGET_SECTION[t.cls]]);
        count[t.cls]++;
        tiles[t.cls] += (t.rows + 63) / 64 * t.tiles_n;
    }
    // buffers of exactly the plan's sizes; the table goes to a copy of its own, as the device copy would
    std::vector<float> kscratch(p.kscratch_floats);
    std::vector<char> dscratch(p.dscratch_bytes);
    std::vector<AdapterWhere> where(p.targets.size());
    std::vector<bf16_t> packed(8);
    for (AdapterWhere& w : where) w = AdapterWhere{packed.data(), packed.data(), 8, 0, 0, 0};
    adapter_table_patch(p, where.data(), (uintptr_t)kscratch.data(), (uintptr_t)dscratch.data());
    std::vector<char> tab(p.table);
    using adapter_detail::row_at;
    for (size_t i = 0; i < p.bytes[SEC_KRON_FACTORS] / sizeof(KronFactorDev); ++i) {
        const KronFactorDev f = row_at<KronFactorDev>(p, SEC_KRON_FACTORS, i);
        REQUIRE((uintptr_t)f.dst % 16 == (uintptr_t)kscratch.data() % 16);
        for (long e = 0; e < (long)f.rows * f.cols; ++e) f.dst[e] += 1.f;
    }
    for (float v : kscratch) REQUIRE(v == 0.f || v == 1.f);   // no two products overlap
    for (size_t i = 0; i < p.bytes[SEC_KRON_TERMS] / sizeof(KronTermDev); ++i) {
        const KronTermDev u = row_at<KronTermDev>(p, SEC_KRON_TERMS, i);
        if (u.w1_f32) REQUIRE(((const float*)u.w1)[(long)u.out_l * u.in_m - 1] == 1.f);
        if (u.w2_f32) REQUIRE(((const float*)u.w2)[(long)u.out_k * u.in_n - 1] == 1.f);
        REQUIRE(!u.wide || (u.in_n % 8 == 0 && u.in_n <= LOKR_TILE_COLS && (uintptr_t)u.w2 % 16 == (u.w2_f32 ? (uintptr_t)kscratch.data() % 16 : 0)));
    }
    for (int sec : {(int)SEC_DORA_LORA_ROWS, (int)SEC_DORA_KRON_ROWS})
        for (size_t i = 0; i < p.bytes[sec] / sizeof(DoraDev); ++i) {
            const DoraDev v = row_at<DoraDev>(p, sec, i);
            for (long e = 0; e < (long)v.n * v.ntiles; ++e) { double d; memcpy(&d, v.part + e, sizeof(d)); d += 1.0; memcpy(v.part + e, &d, sizeof(d)); }
            for (int e = 0; e < v.n; ++e) { float d; memcpy(&d, v.f + e, sizeof(d)); d += 1.f; memcpy(v.f + e, &d, sizeof(d)); }
        }
    for (int sec : {(int)SEC_DORA_LORA_ROWS, (int)SEC_DORA_KRON_ROWS})   // every region written exactly once
        for (size_t i = 0; i < p.bytes[sec] / sizeof(DoraDev); ++i) {
            const DoraDev v = row_at<DoraDev>(p, sec, i);
            double d; memcpy(&d, v.part + (long)v.n * v.ntiles - 1, sizeof(d)); REQUIRE(d == 1.0);
            float f; memcpy(&f, v.f + v.n - 1, sizeof(f)); REQUIRE(f == 1.f);
        }
    for (const AdapterLaunch& l : p.launches) {   // what the launch loop reads
        REQUIRE(l.n > 0 && l.grid_x > 0 && l.grid_y > 0 && l.sec[0] >= 0);
        for (int s : l.sec) REQUIRE(s < ADAPTER_SECTIONS && (s < 0 || p.at[s] + p.bytes[s] <= tab.size()));   // (an empty section may sit at the end: never read)
        const bool merge = l.kernel == ADAPTER_KERNEL_LORA_MERGE || l.kernel == ADAPTER_KERNEL_KRON_MERGE;
        if (merge) {
            REQUIRE((size_t)l.n * sizeof(LoraTargetDev) == p.bytes[l.sec[0]] && (l.pass == 0) == (l.sec[2] < 0));
            if (l.pass) REQUIRE((size_t)l.n * sizeof(DoraDev) == p.bytes[l.sec[2]]);
            const LoraTargetDev last = row_at<LoraTargetDev>(p, l.sec[0], l.n - 1);
            REQUIRE(last.tile0 + (last.rows + 63) / 64 * last.tiles_n == l.grid_x && last.dst == packed.data());
            const size_t term = l.kernel == ADAPTER_KERNEL_LORA_MERGE ? sizeof(LoraTermDev) : sizeof(KronTermDev);
            REQUIRE((size_t)(last.term0 + last.nterms) * term <= p.bytes[l.sec[1]]);
            if (l.kernel == ADAPTER_KERNEL_KRON_MERGE) REQUIRE(l.lds_bytes >= 16 && l.lds_bytes <= LOKR_LDS_FLOATS * 4);
        }
    }
    return 0;
}

int main(int argc, char** argv) {
    REQUIRE(argc == 3);
    std::ifstream in(argv[1]);
    REQUIRE(in.good());
    std::string line, tag, name;
    int listed = 0;
    Call c;
    int want_code = 0;
    long want[5] = {};
    size_t left = 0;
    auto ref = [&](std::istringstream& s) {
        AdapterRef r{};
        s >> r.id >> r.rows >> r.cols >> r.cross >> name;
        c.names.push_back(name);
        r.name = name == "-" ? nullptr : c.names.back().c_str();
        return r;
    };
    while (std::getline(in, line)) {
        std::istringstream s(line);
        s >> tag;
        unsigned long long a, b, w[6];
        if (tag == "call") {
            size_t nl, nk, nd, na;
            s >> nl >> nk >> nd >> na >> want_code >> want[0] >> want[1] >> want[2] >> want[3] >> want[4];
            c = Call{};
            c.names.reserve(nl + nk + nd + na);
            left = nl + nk + nd + na;
        } else if (tag == "L") {
            ace355_lora_term t{};
            c.lref.push_back(ref(s));
            s >> a >> b >> t.rank >> name;
            t.name = c.lref.back().name; t.A_dev = ptr(a); t.B_dev = ptr(b); t.scale = strtof(name.c_str(), nullptr);
            c.lora.push_back(t);
            --left;
        } else if (tag == "K") {
            ace355_kron_term t{};
            c.kref.push_back(ref(s));
            for (auto& x : w) s >> x;
            s >> t.out_l >> t.out_k >> t.in_m >> t.in_n >> t.r1 >> t.r2 >> name;
            t.name = c.kref.back().name; t.scale = strtof(name.c_str(), nullptr);
            t.w1_dev = ptr(w[0]); t.w1a_dev = ptr(w[1]); t.w1b_dev = ptr(w[2]); t.w2_dev = ptr(w[3]); t.w2a_dev = ptr(w[4]); t.w2b_dev = ptr(w[5]);
            c.kron.push_back(t);
            --left;
        } else if (tag == "D") {
            ace355_dora_term t{};
            c.dref.push_back(ref(s));
            std::string eps;
            s >> a >> t.per_input >> eps >> name;
            t.name = c.dref.back().name; t.g_dev = (const float*)ptr(a); t.eps = strtof(eps.c_str(), nullptr); t.multiplier = strtof(name.c_str(), nullptr);
            c.dora.push_back(t);
            --left;
        } else if (tag == "A") {
            c.applied.push_back(ref(s));
            --left;
        } else {
            REQUIRE(!"unknown line");
        }
        if (left == 0) {
            AdapterPlan p;
            REQUIRE(run(c, &p) == want_code);
            if (!want_code)
                REQUIRE((long)p.targets.size() == want[0] && (long)p.launches.size() == want[1] && (long)p.table.size() == want[2] &&
                        (long)p.kscratch_floats == want[3] && (long)p.dscratch_bytes == want[4]);
            ++listed;
        }
    }
    printf("%d listed calls as expected\n", listed);

    // the random sweep
    const int n_random = atoi(argv[2]);
    unsigned long long state = 0x9e3779b97f4a7c15ull;
    auto rnd = [&](int n) { state = state * 6364136223846793005ull + 1442695040888963407ull; return (int)((state >> 33) % (unsigned)n); };
    int refused = 0;
    for (int it = 0; it < n_random; ++it) {
        ace355_dit_config cfg{};
        cfg.hidden_size = 8 * (1 + rnd(40)) + (rnd(50) == 0 ? 4 : 0);   // (rarely not a multiple of 8: a refusal)
        cfg.intermediate_size = 8 * (1 + rnd(100));
        cfg.num_layers = 1 + rnd(4); cfg.num_heads = 1 + rnd(4); cfg.num_kv_heads = 1 + rnd(2);
        Call q;
        const int nl = rnd(6), nk = rnd(6), nd = rnd(4), na = rnd(5);
        q.names.reserve(nl + nk + nd + na);
        const bool sloppy = rnd(4) == 0;   // invalid fields now and then
        auto pick = [&](std::vector<AdapterRef>* refs) {
            const int li = rnd(cfg.num_layers), kind = rnd(PROJ_KINDS);
            q.names.push_back("layers." + std::to_string(li) + ".kind" + std::to_string(kind));
            AdapterRef r = adapter_ref(cfg, q.names.back().c_str(), li, kind);
            if (sloppy && rnd(12) == 0) r.id = -1;
            refs->push_back(r);
            return r;
        };
        auto divisor = [&](long n) { int d = 1 + rnd((int)std::min<long>(n, 64)); while (n % d) --d; return d; };
        const float scales[] = {1.f, 0.f, -0.5f, 1e-4f, INFINITY};
        for (int i = 0; i < nl; ++i) {
            const AdapterRef r = pick(&q.lref);
            q.lora.push_back(ace355_lora_term{sloppy && rnd(20) == 0 ? nullptr : r.name, ptr(16 + rnd(2) * 16 * (!sloppy || rnd(20))), ptr(64),
                                              1 + rnd(80) - (sloppy && rnd(10) == 0 ? 90 : 0), scales[rnd(sloppy ? 5 : 4)]});
        }
        for (int i = 0; i < nk; ++i) {
            const AdapterRef r = pick(&q.kref);
            ace355_kron_term t{};
            t.name = r.name;
            t.out_l = divisor(r.rows); t.out_k = (int)(r.rows / t.out_l) + (sloppy && rnd(10) == 0);
            t.in_m = divisor(r.cols); t.in_n = (int)(r.cols / t.in_m);
            t.r1 = rnd(3) == 0 ? 1 + rnd(70) : 0; t.r2 = rnd(2) == 0 ? 1 + rnd(70) : 0;
            if (t.r1) { t.w1a_dev = ptr(32); t.w1b_dev = ptr(48); } else t.w1_dev = ptr(16);
            if (t.r2) { t.w2a_dev = ptr(32); t.w2b_dev = ptr(48); } else t.w2_dev = ptr(16 + 2 * rnd(8));
            if (sloppy && rnd(10) == 0) t.w2_dev = ptr(16 * rnd(2));
            t.scale = scales[rnd(sloppy ? 5 : 4)];
            q.kron.push_back(t);
        }
        for (int i = 0; i < nd; ++i) {
            const std::vector<AdapterRef>& named = rnd(2) ? q.lref : q.kref;   // mostly beside an additive term
            if (rnd(4) && !named.empty()) q.dref.push_back(named[rnd((int)named.size())]);
            else pick(&q.dref);
            const AdapterRef r = q.dref.back();
            q.dora.push_back(ace355_dora_term{r.name, (const float*)ptr(16 * (!sloppy || rnd(10))), rnd(sloppy ? 3 : 2),
                                              sloppy && rnd(10) == 0 ? -1.f : 0.0078125f * rnd(2), scales[rnd(sloppy ? 5 : 4)]});
        }
        std::vector<int> seen;
        for (int i = 0; i < na; ++i) {   // (the applied set: valid names, each once)
            std::vector<AdapterRef> one;
            const AdapterRef r = pick(&one);
            if (r.id < 0 || std::count(seen.begin(), seen.end(), r.id)) continue;
            seen.push_back(r.id);
            q.applied.push_back(r);
        }
        AdapterPlan p;
        refused += run(q, &p) != 0;
    }
    printf("%d random calls, %d of them refused\n", n_random, refused);
    REQUIRE(n_random < 100 || (refused > n_random / 20 && refused < n_random - n_random / 20));
    return 0;
}
