// tracks_split_check.cpp — drives the host splitter of xm_build_tracks (xm-code_amd/csrc/xm_tracks_split.h, plain C++) on its own, for a run
// under the host sanitizers:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I xm-code_amd/csrc scripts/tracks_split_check.cpp -o /tmp/tracks_split_check
//   /tmp/tracks_split_check [images] [points] [seed]
// It builds a random match graph (every point seen by some images, a few wrong matches), splits it and checks what the contract promises:
// no set sees an image twice, every label is its set's smallest member, and a second run over the shuffled, duplicated edges gives the same
// labels.  Exit status 0 when all of it holds.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "xm_tracks_split.h"

int main(int argc, char **argv) {
    const int n = argc > 1 ? std::atoi(argv[1]) : 40, m = argc > 2 ? std::atoi(argv[2]) : 400;
    std::mt19937_64 rng(argc > 3 ? std::strtoull(argv[3], nullptr, 10) : 7);
    std::vector<int64_t> foff((size_t)n + 1);
    for (int i = 0; i <= n; ++i) foff[(size_t)i] = (int64_t)i * m;   // feature l of image i is point l
    std::vector<uint64_t> edges;
    auto add = [&](int64_t a, int64_t b) { edges.push_back(((uint64_t)std::min(a, b) << 32) | (uint64_t)std::max(a, b)); };
    for (int l = 0; l < m; ++l)
        for (int i = 0; i < n; ++i)
            for (int j = i + 1; j < n; ++j)
                if (rng() % 8 == 0) add(foff[(size_t)i] + l, foff[(size_t)j] + l);
    const size_t right = edges.size();
    for (size_t k = 0; k < right / 50 + 3; ++k) {   // wrong matches: two points, two images
        const int i = (int)(rng() % (uint64_t)n), j = (int)((i + 1 + rng() % (uint64_t)(n - 1)) % (uint64_t)n);
        add(foff[(size_t)i] + (int64_t)(rng() % (uint64_t)m), foff[(size_t)j] + (int64_t)(rng() % (uint64_t)m));
    }
    std::vector<uint64_t> again(edges);
    again.insert(again.end(), edges.begin(), edges.begin() + (std::ptrdiff_t)(edges.size() / 3));   // duplicates
    std::shuffle(again.begin(), again.end(), rng);
    xm::TrackSplit a, b;
    xm::tracks_split(n, foff.data(), edges, a);
    xm::tracks_split(n, foff.data(), again, b);
    int bad = 0;
    if (a.feat != b.feat || a.label != b.label || a.distinct != b.distinct || a.refused != b.refused) { std::printf("the order of the edges changed the result\n"); bad = 1; }
    std::map<int32_t, std::set<int64_t>> seen;
    for (size_t v = 0; v < a.feat.size(); ++v) {
        if (a.label[v] > a.feat[v]) { std::printf("feature %d carries the larger label %d\n", a.feat[v], a.label[v]); bad = 1; }
        if (!seen[a.label[v]].insert(a.feat[v] / m).second) { std::printf("set %d sees image %d twice\n", a.label[v], a.feat[v] / m); bad = 1; }
    }
    for (const auto &s : seen)
        if (!std::binary_search(a.feat.begin(), a.feat.end(), s.first) || a.label[(size_t)(std::lower_bound(a.feat.begin(), a.feat.end(), s.first) - a.feat.begin())] != s.first) {
            std::printf("label %d is not a member of its own set\n", s.first); bad = 1;
        }
    std::printf("%d images, %d points: %lld distinct edges, %zu endpoints, %zu sets, %lld unions refused: %s\n", n, m, (long long)a.distinct, a.feat.size(), seen.size(),
                (long long)a.refused, bad ? "FAILED" : "ok");
    return bad;
}
