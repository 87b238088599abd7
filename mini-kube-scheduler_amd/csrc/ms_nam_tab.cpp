// ms_nam_tab.cpp — MS_PLUGINS_NU_NN_NAM's registered term sets: the lookup
// tables (NamTab, ms_nam_layout.h) built on the host from the preferred and
// required sets, and the three configuration calls that install them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "ms_ctx.h"
#include "ms_nam_layout.h"

using namespace msgpu;

// Set id's lookup table (NamTab) from its preferred term set and its required
// set (either may be null: the id is past that table). Preferred term k: bit k of
// z[v] / l[v]; required term k: bit 4 + k; no requirement: kNamNoReqBit on every
// value id of both keys (every node passes).
static NamTab nam_tab_of(const ms_nam_term_set_ext *x, const ms_nam_required_set *q) {
    NamTab t{};
    auto holds = [](const uint32_t *mask, uint32_t v) { return (mask[v >> 5] >> (v & 31u)) & 1u; };
    for (int k = 0; x && k < MS_NAM_TERMS; ++k) {
        const ms_pref_term_ext &e = x->term[k];
        if (e.weight == 0) continue;
        for (uint32_t v = 0; v < 256u; ++v) {
            if (holds(e.mask[0], v)) t.z[v] |= (uint8_t)(1u << k);
            if (holds(e.mask[1], v)) t.l[v] |= (uint8_t)(1u << k);
        }
    }
    for (uint32_t m = 0; m < 16u; ++m) {
        uint32_t w = 0;
        for (int k = 0; x && k < MS_NAM_TERMS; ++k)
            if ((m >> k) & 1u) w += x->term[k].weight;
        t.wsum[m] = (uint16_t)w;
    }
    const uint32_t n_req = q ? q->n_terms : 0u;
    for (uint32_t v = 0; v < 256u; ++v) {
        if (n_req == 0) {
            t.z[v] |= (uint8_t)kNamNoReqBit;
            t.l[v] |= (uint8_t)kNamNoReqBit;
        }
        for (uint32_t k = 0; k < n_req; ++k) {
            if (holds(q->term[k].mask[0], v)) t.z[v] |= (uint8_t)(kNamNoReqBit << k);
            if (holds(q->term[k].mask[1], v)) t.l[v] |= (uint8_t)(kNamNoReqBit << k);
        }
    }
    return t;
}

// ms_nam_term_set's {key, value} terms: In [value] (1..254) or Exists (0xFF) on
// one key, all ids on the other; value 0 ("unlabelled") never matches.
static ms_nam_term_set_ext nam_ext_of(const ms_nam_term_set &x) {
    ms_nam_term_set_ext e{};
    for (int k = 0; k < MS_NAM_TERMS; ++k) {
        const ms_pref_term &t = x.term[k];
        if (t.weight == 0 || t.value == 0) continue;
        ms_pref_term_ext &o = e.term[k];
        const int key = t.key ? 1 : 0;
        for (int w = 0; w < 8; ++w) o.mask[1 - key][w] = ~0u;
        if (t.value == 0xFFu) {
            for (int w = 0; w < 8; ++w) o.mask[key][w] = ~0u;
            o.mask[key][0] &= ~1u;
        } else {
            o.mask[key][t.value >> 5] |= 1u << (t.value & 31u);
        }
        o.weight = t.weight;
    }
    return e;
}

// Installs the context's tables after one of them was replaced (pref / req: the
// new one, or null to keep the registered one): a NamTab for each of
// max(preferred sets, required sets) ids, built from the host copies of both.
static int nam_install(ms_ctx *c, std::vector<ms_nam_term_set_ext> *pref, std::vector<ms_nam_required_set> *req,
                       const char *who) {
    std::lock_guard<std::mutex> g(c->sched_mu);
    if (pref) c->h_pref.swap(*pref);
    if (req) c->h_req.swap(*req);
    const uint32_t n_pref = (uint32_t)c->h_pref.size(), n_req = (uint32_t)c->h_req.size();
    const uint32_t n_sets = std::max(n_pref, n_req);
    std::vector<NamTab> tabs(n_sets);
    for (uint32_t i = 0; i < n_sets; ++i)
        tabs[i] = nam_tab_of(i < n_pref ? &c->h_pref[i] : nullptr, i < n_req ? &c->h_req[i] : nullptr);
    MS_HIP(c, hipSetDevice(c->cfg.device));
    MS_HIP(c, hipDeviceSynchronize());  // (no cycle still reads the previous table; a configuration call)
    if (n_sets > c->terms_cap) {
        c->terms_cap = c->n_terms = 0;  // (no table, no sets, should the allocation fail)
        if (!c->d_terms.alloc((size_t)n_sets * sizeof(NamTab)))
            return fail(c, MS_E_OOM, std::string(who) + ": term table");
        c->terms_cap = n_sets;
    }
    if (n_sets) MS_HIP(c, hipMemcpy(c->d_terms, tabs.data(), (size_t)n_sets * sizeof(NamTab), hipMemcpyHostToDevice));
    c->n_terms = n_sets;
    return MS_OK;
}

extern "C" {

int ms_nam_term_sets(ms_ctx *c, uint32_t n_sets, const ms_nam_term_set *sets) {
    if (!c || (n_sets && !sets) || n_sets > 0xFFFFu) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NN_NAM)
        return fail(c, MS_E_INVAL, "ms_nam_term_sets: the multi-term NodeAffinity plugin set only");
    std::vector<ms_nam_term_set_ext> pref(n_sets);
    for (uint32_t i = 0; i < n_sets; ++i) {
        for (int k = 0; k < MS_NAM_TERMS; ++k) {
            const ms_pref_term &x = sets[i].term[k];
            if (x.key > 1 || x.weight > 100)
                return fail(c, MS_E_INVAL, "ms_nam_term_sets: term key must be 0 or 1 and weight 0..100");
            // (value 0xFF is Exists; an In term names a value id 1..254, so a node label id
            // of 255 matches Exists only: ZoneIds hands out at most 254 ids)
        }
        pref[i] = nam_ext_of(sets[i]);
    }
    return nam_install(c, &pref, nullptr, "ms_nam_term_sets");
}

int ms_nam_term_sets_ext(ms_ctx *c, uint32_t n_sets, const ms_nam_term_set_ext *sets) {
    if (!c || (n_sets && !sets) || n_sets > 0xFFFFu) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NN_NAM)
        return fail(c, MS_E_INVAL, "ms_nam_term_sets_ext: the multi-term NodeAffinity plugin set only");
    for (uint32_t i = 0; i < n_sets; ++i)
        for (int k = 0; k < MS_NAM_TERMS; ++k)
            if (sets[i].term[k].weight > 100) return fail(c, MS_E_INVAL, "ms_nam_term_sets_ext: weight 0..100");
    std::vector<ms_nam_term_set_ext> pref(sets, sets + n_sets);
    return nam_install(c, &pref, nullptr, "ms_nam_term_sets_ext");
}

int ms_nam_required_sets(ms_ctx *c, uint32_t n_sets, const ms_nam_required_set *sets) {
    if (!c || (n_sets && !sets) || n_sets > 0xFFFFu) return MS_E_INVAL;
    if (c->cfg.plugin_set != MS_PLUGINS_NU_NN_NAM)
        return fail(c, MS_E_INVAL, "ms_nam_required_sets: the multi-term NodeAffinity plugin set only");
    for (uint32_t i = 0; i < n_sets; ++i)
        if (sets[i].n_terms > MS_NAM_REQ_TERMS)
            return fail(c, MS_E_INVAL, "ms_nam_required_sets: at most MS_NAM_REQ_TERMS terms per set");
    std::vector<ms_nam_required_set> req(sets, sets + n_sets);
    return nam_install(c, nullptr, &req, "ms_nam_required_sets");
}

}  // extern "C"
