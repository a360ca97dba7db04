// xm_tracks_split.h — the XM_TRACKS_SPLIT policy of xm_build_tracks (include/xm_amd.h, rule 4) on the host: plain C++, no device code, so that
// it can be compiled and run on its own.  The distinct edges, sorted as (smaller id, larger id), are visited one by one; two roots are
// united when their image sets are disjoint, the larger root under the smaller.  A set of one member carries its image alone; larger sets
// keep a sorted image list at their root, and of two lists the shorter is the one that is walked.
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace xm {

struct TrackSplit {
    std::vector<int32_t> feat;    // the endpoints, ascending
    std::vector<int32_t> label;   // per endpoint: the smallest member of its set
    int64_t distinct = 0, refused = 0;
};

// edges: (smaller id << 32 | larger id) words in any order, duplicates allowed (sorted and made unique in place); every id < foff[n]
inline void tracks_split(int64_t n, const int64_t *foff, std::vector<uint64_t> &edges, TrackSplit &out) {
    out = TrackSplit();
    std::sort(edges.begin(), edges.end());
    edges.erase(std::unique(edges.begin(), edges.end()), edges.end());
    out.distinct = (int64_t)edges.size();
    // the endpoints, ascending: the smaller ends come sorted with the edges, the larger ends are sorted on their own
    std::vector<int32_t> &verts = out.feat;
    std::vector<int32_t> lo, hi;
    lo.reserve(edges.size()); hi.reserve(edges.size());
    for (const uint64_t e : edges) {
        const int32_t u = (int32_t)(e >> 32);
        if (lo.empty() || lo.back() != u) lo.push_back(u);
        hi.push_back((int32_t)(e & 0xffffffffull));
    }
    std::sort(hi.begin(), hi.end());
    hi.erase(std::unique(hi.begin(), hi.end()), hi.end());
    verts.resize(lo.size() + hi.size());
    verts.erase(std::set_union(lo.begin(), lo.end(), hi.begin(), hi.end(), verts.begin()), verts.end());
    const size_t nv = verts.size();
    // per endpoint: its parent, its image, and -- once its set has more than one member -- the set's sorted image list (at the root)
    std::vector<int32_t> parent(nv), image(nv), list_of(nv, -1);
    std::vector<std::vector<int32_t>> lists;
    int64_t img = 0;
    for (size_t v = 0; v < nv; ++v) {
        parent[v] = (int32_t)v;
        while (img + 1 < n && foff[img + 1] <= (int64_t)verts[v]) ++img;   // (ascending endpoints: the image only moves forward; at most n steps in all)
        image[v] = (int32_t)img;
    }
    auto find = [&](int32_t v) {
        while (parent[v] != v) { parent[v] = parent[parent[v]]; v = parent[v]; }   // path halving: parents only ever fall
        return v;
    };
    auto has = [&](int32_t root, int32_t im) {
        if (list_of[root] < 0) return image[root] == im;
        const std::vector<int32_t> &l = lists[(size_t)list_of[root]];
        return std::binary_search(l.begin(), l.end(), im);
    };
    auto shares = [&](int32_t a, int32_t b) {   // walks the shorter list
        if (list_of[a] < 0) return has(b, image[a]);
        if (list_of[b] < 0) return has(a, image[b]);
        const std::vector<int32_t> &la = lists[(size_t)list_of[a]], &lb = lists[(size_t)list_of[b]];
        const int32_t longer = la.size() <= lb.size() ? b : a;
        for (const int32_t im : la.size() <= lb.size() ? la : lb)
            if (has(longer, im)) return true;
        return false;
    };
    std::vector<int32_t> merged;
    size_t iu = 0;
    for (const uint64_t e : edges) {
        const int32_t u = (int32_t)(e >> 32), v = (int32_t)(e & 0xffffffffull);
        while (verts[iu] != u) ++iu;   // (the edges are sorted by their smaller end: its index only moves forward)
        const int32_t ru = find((int32_t)iu), rv = find((int32_t)(std::lower_bound(verts.begin(), verts.end(), v) - verts.begin()));
        if (ru == rv) continue;
        if (shares(ru, rv)) { out.refused += 1; continue; }
        const int32_t a = std::min(ru, rv), b = std::max(ru, rv);   // (the endpoints are ascending: the smaller index is the smaller id)
        const int32_t one_a = image[a], one_b = image[b];
        const std::vector<int32_t> *la = list_of[a] < 0 ? nullptr : &lists[(size_t)list_of[a]], *lb = list_of[b] < 0 ? nullptr : &lists[(size_t)list_of[b]];
        merged.resize((la ? la->size() : 1) + (lb ? lb->size() : 1));
        std::merge(la ? la->data() : &one_a, la ? la->data() + la->size() : &one_a + 1, lb ? lb->data() : &one_b, lb ? lb->data() + lb->size() : &one_b + 1,
                   merged.begin());
        int32_t slot = list_of[a] >= 0 ? list_of[a] : list_of[b];   // an existing list is taken over
        if (slot < 0) { slot = (int32_t)lists.size(); lists.emplace_back(); }
        else if (list_of[a] >= 0 && list_of[b] >= 0) std::vector<int32_t>().swap(lists[(size_t)list_of[b]]);
        lists[(size_t)slot].swap(merged);
        list_of[a] = slot; list_of[b] = -1;
        parent[b] = a;
    }
    out.label.resize(nv);
    for (size_t v = 0; v < nv; ++v) out.label[v] = verts[(size_t)find((int32_t)v)];
}

}  // namespace xm
