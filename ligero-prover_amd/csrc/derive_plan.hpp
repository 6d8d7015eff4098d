// derive_plan.hpp -- the host-side rules of derived slots (lig_hip.h: lig_derived_check, lig_rows_set_derived): which lists are accepted,
// the wave of every listed slot, and the compact constraint-major program the kernels of derive.hip walk -- per wave the targets (slot,
// sign, right-hand-side index, term range) and their OTHER terms as (slot, coefficient index) -- next to a copy of the coefficient table.
// An entry {slot, LIG_DERIVED_PRODUCT} is a PRODUCT entry: column i of a LIG_ELEM_PRODUCT row, which reads the two operand slots in front
// of it instead of the terms of a constraint; it shares the wave numbering and is laid out in a list of its own (DeriveProduct).
// The system has passed lig_linear_check against the same kinds: every term's slot lies on a LINEAR / QX / QY / QZ row below `rows`,
// every coefficient index is one of the two specials or < n_coefs, rows * l < 2^32.
// Host only: nothing but lig_hip.h and the standard library, so that a plain host compiler builds it (tests/cpp/derive_plan_prog.cpp).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <utility>
#include <vector>

#include "../../include/lig_hip.h"

namespace lig {
// A target with at most this many other terms is one lane's work (2 to 4 terms for an eval of a few witnesses, 33 for a machine word
// recomposed from bits); one with more is summed by a whole workgroup of k_derive_wave, as k_diag_lin_heavy sums a long constraint.
static constexpr uint32_t DERIVE_LANE_MAX = 64;
static constexpr uint32_t DERIVE_RHS_ZERO = 0xFFFFFFFDu;      // DeriveTarget.rhs: b_c = 0 (a coefficient index is < n_coefs <= 0xFFFFFFFD or a special)

// one derived slot of the program: w[slot] = b - sum (negate == 0: the slot has coefficient +1 in its constraint) or sum - b (negate == 1:
// coefficient -1), sum = the sum of a * w over terms [begin, end) of the program's term list, b = the table entry `rhs` (or a special)
struct DeriveTarget { uint32_t slot, negate, rhs, begin, end; };
static_assert(sizeof(DeriveTarget) == 20, "the kernel of derive.hip reads these 20 bytes");

// one PRODUCT entry of the program ({slot, LIG_DERIVED_PRODUCT}): column `col` of the LIG_ELEM_PRODUCT row `row`, re-formed from the
// expanded matrix as w[row - 2][col] * w[row - 1][col].  row is global in DerivePlan and local in DeriveShardPlan (the deal never splits
// a triple: the operand rows are the two local rows in front).  Checked here: 2 <= row < rows, col < l.
struct DeriveProduct { uint32_t row, col; };
static_assert(sizeof(DeriveProduct) == 8, "the kernel of derive.hip reads these 8 bytes");

struct DerivePlan {
    uint32_t n_waves = 0;
    std::vector<uint32_t> wave_of;        // per entry of the caller's list, linear and product alike: 1 .. n_waves
    // wave w (0-based) owns targets [wave_begin[w], wave_begin[w + 1]): first its wave_light[w] targets with at most DERIVE_LANE_MAX other
    // terms, then the heavy ones; within each class in the order of the caller's list.  Linear entries only.
    std::vector<uint32_t> wave_begin, wave_light;
    std::vector<DeriveTarget> targets;
    std::vector<lig_lin_term> terms;      // the other terms of every target, in the order of its constraint
    std::vector<uint8_t> coefs;           // sys.coefs as passed: n_coefs x 32 bytes, canonical
    // the product entries: wave w owns products [prod_begin[w], prod_begin[w + 1]), in the order of the caller's list (n_waves + 1 offsets)
    std::vector<uint32_t> prod_begin;
    std::vector<DeriveProduct> products;
    uint64_t n_terms() const { return terms.size() + 2 * (uint64_t)products.size(); }      // lig_derived_info.n_terms: a product reads its two operands
};

// nullptr = accepted (out is the program), else why not (out is unspecified).  d may be in any order; n == 0 is the empty program.
// elem_bytes: one per row as in lig_rows_job, or NULL (no row is derived).
inline const char* plan_derived(const lig_linear_system& sys, const uint8_t* kinds, uint64_t rows, uint32_t l, const uint8_t* elem_bytes,
                                const lig_derived_slot* d, uint64_t n, DerivePlan& out) {
    out = DerivePlan{};
    out.wave_begin.assign(1, 0);
    out.prod_begin.assign(1, 0);
    if (!n) return nullptr;
    if (!d) return "null list";
    if (n >= (1ull << 32)) return "too many derived slots";
    std::unordered_map<uint32_t, uint32_t> index;      // derived slot -> its entry in d
    index.reserve((size_t)n * 2);
    for (uint64_t i = 0; i < n; i++)
        if (!index.emplace(d[i].slot, (uint32_t)i).second) return "a slot is listed twice";
    auto is_product = [&](uint64_t i) { return d[i].constraint == LIG_DERIVED_PRODUCT; };
    // is column `col` of the LIG_ELEM_PRODUCT row `row` re-formed by a product entry of this list?
    auto reformed = [&](uint64_t row, uint32_t col) {
        const auto it = index.find((uint32_t)(row * l + col));
        return it != index.end() && is_product(it->second);
    };
    std::vector<uint32_t> at(n);                        // the term of the defining constraint that is the target (linear entries)
    for (uint64_t i = 0; i < n; i++) {
        const uint64_t row = d[i].slot / l;
        const uint32_t col = d[i].slot % l;
        if (is_product(i)) {
            if (row >= rows) return "a product entry beyond the rows";
            if (!elem_bytes || elem_bytes[row] != LIG_ELEM_PRODUCT) return "a product entry on a row that is not LIG_ELEM_PRODUCT";
            if (row < 2 || (kinds[row] & 0x7f) != LIG_ROW_QZ || (kinds[row - 2] & 0x7f) != LIG_ROW_QX || (kinds[row - 1] & 0x7f) != LIG_ROW_QY)
                return "a product entry on a row that is not the QZ row of a triple";
            continue;
        }
        if (d[i].constraint >= sys.n_constraints) return "a defining constraint is not a constraint of the system";
        const uint32_t b = sys.term_begin[d[i].constraint], e = sys.term_begin[d[i].constraint + 1];
        uint32_t hits = 0;
        for (uint32_t t = b; t < e; t++)
            if (sys.terms[t].slot == d[i].slot) { hits++; at[i] = t; }
        if (hits != 1) return hits ? "a target occurs more than once in its defining constraint" : "a target does not occur in its defining constraint";
        const uint32_t coef = sys.terms[at[i]].coef;
        if (coef != LIG_COEF_ONE && coef != LIG_COEF_NEG_ONE) return "the coefficient of a target must be LIG_COEF_ONE or LIG_COEF_NEG_ONE";
        if (row >= rows) return "a target beyond the rows";      // (< rows: the slot is a term of a checked system)
        if (elem_bytes) {
            if (elem_bytes[row] == LIG_ELEM_PRODUCT) return "a target on a LIG_ELEM_PRODUCT row";
            // the row's own product is formed from the PACKED operand rows: a value derived here reaches it only through a product entry
            // of the same column, which re-forms it from the matrix
            const uint8_t kd = kinds[row] & 0x7f;
            if (kd == LIG_ROW_QX && row + 2 < rows && elem_bytes[row + 2] == LIG_ELEM_PRODUCT && !reformed(row + 2, col)) return "a target is an operand slot of a LIG_ELEM_PRODUCT row";
            if (kd == LIG_ROW_QY && row + 1 < rows && elem_bytes[row + 1] == LIG_ELEM_PRODUCT && !reformed(row + 1, col)) return "a target is an operand slot of a LIG_ELEM_PRODUCT row";
        }
    }
    // what entry i reads, as a range of positions: the terms of its defining constraint (its own term skipped), or the two operands of a
    // product entry
    auto reads_begin = [&](uint32_t i) { return is_product(i) ? 0u : sys.term_begin[d[i].constraint]; };
    auto reads_end = [&](uint32_t i) { return is_product(i) ? 2u : sys.term_begin[d[i].constraint + 1]; };
    auto read_slot = [&](uint32_t i, uint32_t t) { return is_product(i) ? d[i].slot - (2 - t) * l : sys.terms[t].slot; };
    // waves: 1 + the largest wave among the derived slots an entry reads (0 for a slot that is not derived); depth-first with an explicit
    // stack, a slot met again while it is still open closes a cycle
    out.wave_of.assign(n, 0);
    std::vector<uint8_t> state(n, 0);                   // 0 untouched, 1 open, 2 done
    std::vector<std::pair<uint32_t, uint32_t>> stack;   // (entry, next position to look at)
    for (uint64_t root = 0; root < n; root++) {
        if (state[root]) continue;
        state[root] = 1;
        stack.emplace_back((uint32_t)root, reads_begin((uint32_t)root));
        while (!stack.empty()) {
            const uint32_t i = stack.back().first, e = reads_end(i);
            uint32_t& t = stack.back().second;
            bool descended = false;
            for (; t < e; t++) {
                if (!is_product(i) && t == at[i]) continue;
                const auto it = index.find(read_slot(i, t));
                if (it == index.end()) continue;
                const uint32_t j = it->second;
                if (state[j] == 1) return "the derived slots form a cycle";
                if (state[j] == 0) { state[j] = 1; stack.emplace_back(j, reads_begin(j)); descended = true; break; }      // (t stays: looked at again when j is done)
                out.wave_of[i] = std::max(out.wave_of[i], out.wave_of[j]);
            }
            if (descended) continue;
            out.wave_of[i] += 1;
            if (out.wave_of[i] > LIG_DERIVE_MAX_WAVES) return "more than LIG_DERIVE_MAX_WAVES waves";
            state[i] = 2;
            stack.pop_back();
        }
    }
    for (uint64_t i = 0; i < n; i++) out.n_waves = std::max(out.n_waves, out.wave_of[i]);
    // the program: wave-major, light targets in front of the heavy ones; the product entries of a wave in a list of their own
    auto others = [&](uint64_t i) { return sys.term_begin[d[i].constraint + 1] - sys.term_begin[d[i].constraint] - 1; };
    out.wave_begin.assign((size_t)out.n_waves + 1, 0);
    out.wave_light.assign(out.n_waves, 0);
    out.prod_begin.assign((size_t)out.n_waves + 1, 0);
    uint64_t n_linear = 0;
    for (uint64_t i = 0; i < n; i++) {
        if (is_product(i)) { out.prod_begin[out.wave_of[i]]++; continue; }
        n_linear++;
        out.wave_begin[out.wave_of[i]]++;
        if (others(i) <= DERIVE_LANE_MAX) out.wave_light[out.wave_of[i] - 1]++;
    }
    for (uint32_t w = 0; w < out.n_waves; w++) { out.wave_begin[w + 1] += out.wave_begin[w]; out.prod_begin[w + 1] += out.prod_begin[w]; }
    std::vector<uint32_t> light_at(out.n_waves), heavy_at(out.n_waves), prod_at(out.prod_begin.begin(), out.prod_begin.end() - 1);
    for (uint32_t w = 0; w < out.n_waves; w++) { light_at[w] = out.wave_begin[w]; heavy_at[w] = out.wave_begin[w] + out.wave_light[w]; }
    out.targets.resize(n_linear);
    out.products.resize(n - n_linear);
    std::vector<uint32_t> entry_of(n_linear);           // program position -> entry of d
    uint64_t total = 0;
    for (uint64_t i = 0; i < n; i++) {
        const uint32_t w = out.wave_of[i] - 1;
        if (is_product(i)) { out.products[prod_at[w]++] = DeriveProduct{d[i].slot / l, d[i].slot % l}; continue; }
        entry_of[others(i) <= DERIVE_LANE_MAX ? light_at[w]++ : heavy_at[w]++] = (uint32_t)i;
        total += others(i);
    }
    out.terms.reserve(total);
    for (uint64_t p = 0; p < n_linear; p++) {
        const uint32_t i = entry_of[p], c = d[i].constraint;
        DeriveTarget tg;
        tg.slot = d[i].slot;
        tg.negate = sys.terms[at[i]].coef == LIG_COEF_NEG_ONE ? 1u : 0u;
        tg.rhs = DERIVE_RHS_ZERO;
        if (sys.n_rhs) {
            const uint32_t* const rend = sys.rhs_constraint + sys.n_rhs;
            const uint32_t* rc = std::lower_bound(sys.rhs_constraint, rend, c);      // strictly ascending (lig_linear_check)
            if (rc != rend && *rc == c) tg.rhs = sys.rhs_coef[rc - sys.rhs_constraint];
        }
        tg.begin = (uint32_t)out.terms.size();
        for (uint32_t t = sys.term_begin[c]; t < sys.term_begin[c + 1]; t++)
            if (t != at[i]) out.terms.push_back(sys.terms[t]);
        tg.end = (uint32_t)out.terms.size();
        out.targets[p] = tg;
    }
    if (sys.n_coefs) out.coefs.assign(sys.coefs, sys.coefs + sys.n_coefs * 32);
    return nullptr;
}

// ---- the same list on a rows shard (lig_shard_rows_set_derived): one rank's program and the exchange schedule of all ranks
//
// The rows are dealt over `world` ranks; a target is formed by the rank that was dealt its row, from terms that lie on its own rows (LOCAL
// terms) and on rows of other ranks (IMPORTED terms, some of them derived there in an earlier wave).  Every rank has the whole list and
// the deal, so every rank computes the same schedule: E_q(w) = the distinct slots of rank q that a wave-w target of ANOTHER rank reads and
// that no earlier wave has shipped, ascending.  The exchange of wave w is one all-gather of B(w) = max_q |E_q(w)| elements per rank; a wave
// with B(w) = 0 has none, on every rank alike.  The import buffer is absolute over the commit: slot E_q(w)[i] lies at
// import_begin[w] + q * B(w) + i.  A slot is shipped once, in the first wave that reads it across ranks; a derived slot of wave v is read
// only by waves after v, so its value is final by then.

// one derived slot a rank forms: local row and column of the target, then as DeriveTarget; terms [begin, mid) are local (slot = local row
// * l + col in the rank's matrix), terms [mid, end) imported (slot = position in the import buffer)
struct DeriveShardTarget { uint32_t row, col, negate, rhs, begin, mid, end; };
static_assert(sizeof(DeriveShardTarget) == 28, "the kernel of derive.hip reads these 28 bytes");

// the deal as the plan reads it: per global row the rank that was dealt it and its row index there.  Local rows are in commit order, so
// the index is the number of earlier rows of the same rank.
struct DeriveDeal { std::vector<uint32_t> owner, local_of; };
inline DeriveDeal derive_deal_of(const std::vector<uint32_t>& owner, uint32_t world) {
    DeriveDeal dl;
    dl.owner = owner;
    dl.local_of.resize(owner.size());
    std::vector<uint32_t> held(world, 0);
    for (size_t r = 0; r < owner.size(); r++) dl.local_of[r] = held[owner[r]]++;
    return dl;
}

struct DeriveShardPlan {
    uint32_t n_waves = 0, n_exchanges = 0;                 // waves of the whole list; those with B(w) > 0
    std::vector<uint32_t> wave_begin, wave_light;          // THIS rank's targets per wave, light ones in front (as DerivePlan)
    std::vector<DeriveShardTarget> targets;
    std::vector<lig_lin_term> terms;
    std::vector<uint32_t> block, import_begin;             // B(w); first element of wave w's blocks in the import buffer (+1 entry = its size)
    // E_q(w) of every rank, global slots: sends[send_begin[q * n_waves + w] .. send_begin[q * n_waves + w + 1])
    std::vector<uint32_t> send_begin, sends;
    std::vector<uint32_t> export_begin, exports;           // E_rank(w) as local slots (n_waves + 1 offsets): what k_derive_export reads
    uint64_t local_terms = 0, imported_terms = 0, n_imports = 0, n_exports = 0;      // n_imports: distinct foreign slots this rank reads
    // THIS rank's product entries per wave (n_waves + 1 offsets), local rows: a triple is dealt whole, so a product entry is formed by the
    // rank that holds its row from two local operands and never imports; local_terms counts it as 2
    std::vector<uint32_t> prod_begin;
    std::vector<DeriveProduct> products;
    uint64_t local_targets() const { return targets.size() + products.size(); }
    uint64_t import_elems() const { return import_begin.empty() ? 0 : import_begin.back(); }
};

// nullptr = planned, else why not.  P: the accepted program of plan_derived over the whole trace; deal: one entry per row of that trace,
// every owner < world.
inline const char* plan_derived_shard(const DerivePlan& P, const DeriveDeal& deal, uint32_t l, uint32_t rank, uint32_t world, DeriveShardPlan& out) {
    out = DeriveShardPlan{};
    const uint32_t NW = P.n_waves;
    out.n_waves = NW;
    out.wave_begin.assign((size_t)NW + 1, 0);
    out.wave_light.assign(NW, 0);
    out.block.assign(NW, 0);
    out.import_begin.assign((size_t)NW + 1, 0);
    out.send_begin.assign((size_t)world * NW + 1, 0);
    out.export_begin.assign((size_t)NW + 1, 0);
    out.prod_begin.assign((size_t)NW + 1, 0);
    if (!world || rank >= world) return "rank >= world";
    const size_t rows = deal.owner.size();
    auto row_of = [&](uint32_t slot) { return (size_t)(slot / l); };
    std::unordered_map<uint32_t, uint32_t> position;       // shipped slot -> its place in the import buffer
    std::vector<std::vector<uint32_t>> per_rank(world);    // the wave in hand: E_q(w)
    std::vector<std::vector<uint32_t>> sends_of((size_t)world * NW);
    std::unordered_map<uint32_t, uint8_t> read_here;       // distinct foreign slots of THIS rank's targets
    for (uint32_t w = 0; w < NW; w++) {
        for (auto& v : per_rank) v.clear();
        for (uint32_t p = P.wave_begin[w]; p < P.wave_begin[w + 1]; p++) {
            const DeriveTarget& tg = P.targets[p];
            if (row_of(tg.slot) >= rows) return "a target beyond the deal";
            const uint32_t holder = deal.owner[row_of(tg.slot)];
            for (uint32_t t = tg.begin; t < tg.end; t++) {
                const uint32_t s = P.terms[t].slot;
                if (row_of(s) >= rows) return "a term beyond the deal";
                const uint32_t q = deal.owner[row_of(s)];
                if (q >= world) return "a row dealt to a rank >= world";
                if (q != holder && !position.count(s)) per_rank[q].push_back(s);
            }
        }
        uint64_t widest = 0;
        for (uint32_t q = 0; q < world; q++) {
            std::vector<uint32_t>& v = per_rank[q];
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
            widest = std::max<uint64_t>(widest, v.size());
        }
        const uint64_t next = (uint64_t)out.import_begin[w] + widest * world;
        if (next >= (1ull << 32)) return "the exchange needs 2^32 elements or more";
        out.block[w] = (uint32_t)widest;
        out.import_begin[w + 1] = (uint32_t)next;
        if (widest) out.n_exchanges++;
        for (uint32_t q = 0; q < world; q++) {
            for (size_t i = 0; i < per_rank[q].size(); i++) position.emplace(per_rank[q][i], (uint32_t)(out.import_begin[w] + (uint64_t)q * widest + i));
            sends_of[(size_t)q * NW + w] = per_rank[q];
        }
        // this rank's share of the wave: what it sends, then what it forms
        for (const uint32_t s : per_rank[rank]) out.exports.push_back(deal.local_of[row_of(s)] * l + s % l);
        out.export_begin[w + 1] = (uint32_t)out.exports.size();
        for (uint32_t p = P.wave_begin[w]; p < P.wave_begin[w + 1]; p++) {
            const DeriveTarget& tg = P.targets[p];
            if (deal.owner[row_of(tg.slot)] != rank) continue;
            DeriveShardTarget st;
            st.row = deal.local_of[row_of(tg.slot)];
            st.col = tg.slot % l;
            st.negate = tg.negate;
            st.rhs = tg.rhs;
            st.begin = (uint32_t)out.terms.size();
            for (uint32_t t = tg.begin; t < tg.end; t++) {
                const lig_lin_term tm = P.terms[t];
                if (deal.owner[row_of(tm.slot)] == rank) out.terms.push_back(lig_lin_term{deal.local_of[row_of(tm.slot)] * l + tm.slot % l, tm.coef});
            }
            st.mid = (uint32_t)out.terms.size();
            for (uint32_t t = tg.begin; t < tg.end; t++) {
                const lig_lin_term tm = P.terms[t];
                if (deal.owner[row_of(tm.slot)] == rank) continue;
                out.terms.push_back(lig_lin_term{position.at(tm.slot), tm.coef});      // (shipped in this wave at the latest)
                read_here.emplace(tm.slot, 1);
            }
            st.end = (uint32_t)out.terms.size();
            out.local_terms += st.mid - st.begin;
            out.imported_terms += st.end - st.mid;
            if (p - P.wave_begin[w] < P.wave_light[w]) out.wave_light[w]++;
            out.targets.push_back(st);
        }
        out.wave_begin[w + 1] = (uint32_t)out.targets.size();
        // the product entries of the wave: both operands lie on the two local rows in front of the target's (a re-formed slot that a target
        // of another rank reads travels like any other slot, in the first wave that reads it across ranks -- a later one than this)
        for (uint32_t p = P.prod_begin[w]; p < P.prod_begin[w + 1]; p++) {
            const DeriveProduct pr = P.products[p];
            if (pr.row >= rows || pr.row < 2) return "a product entry beyond the deal";
            const uint32_t holder = deal.owner[pr.row];
            if (holder >= world) return "a row dealt to a rank >= world";
            if (deal.owner[pr.row - 2] != holder || deal.owner[pr.row - 1] != holder || deal.local_of[pr.row] != deal.local_of[pr.row - 2] + 2)
                return "the deal splits the triple of a product entry";
            if (holder != rank) continue;
            out.products.push_back(DeriveProduct{deal.local_of[pr.row], pr.col});
            out.local_terms += 2;
        }
        out.prod_begin[w + 1] = (uint32_t)out.products.size();
    }
    for (size_t i = 0; i < sends_of.size(); i++) {
        out.sends.insert(out.sends.end(), sends_of[i].begin(), sends_of[i].end());
        out.send_begin[i + 1] = (uint32_t)out.sends.size();
    }
    out.n_imports = read_here.size();
    out.n_exports = out.exports.size();
    return nullptr;
}
}  // namespace lig
