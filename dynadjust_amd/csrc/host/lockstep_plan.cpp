// The schedule of the lock-step chains (a.chain_runs), planned without the device: which networks and runs, and every
// step of the three levels in the order of the plan's batches -- the runs merged to their end stations, the junction matrices at the
// runs' boundaries by a scan over spans of runs, both chains inside every run.  A step names the matrices it reads and writes (a block's
// red / jfwd / jrev, or merged system i); dna_adjust::PrepareLockstepChains makes the merged systems and the plan.
#include <algorithm>
#include <map>
#include <numeric>
#include <set>

#include "dna_adjust.hpp"

namespace dynadjust {
namespace networkadjust {

namespace {

std::vector<UINT32> sorted_union(std::vector<UINT32> a, const std::vector<UINT32>& b) {
    a.insert(a.end(), b.begin(), b.end());
    std::sort(a.begin(), a.end());
    a.erase(std::unique(a.begin(), a.end()), a.end());
    return a;
}

long position(const std::vector<UINT32>& sorted, UINT32 g) {
    auto it = std::lower_bound(sorted.begin(), sorted.end(), g);
    return (it != sorted.end() && *it == g) ? (long)(it - sorted.begin()) : -1L;
}

// the positions of `ids` in `sorted`, appended to `out`; false: one of them is not there
bool positions_in(const std::vector<UINT32>& sorted, const std::vector<UINT32>& ids, std::vector<UINT32>& out) {
    for (UINT32 s : ids) {
        const long q = position(sorted, s);
        if (q < 0) return false;
        out.push_back((UINT32)q);
    }
    return true;
}

}  // namespace

struct dna_adjust::lock_scheduler {
    using ref = lock_ref_t;
    struct run_t {
        UINT32 a, b, s, e;                   // its blocks; its network's blocks
        int first, last;                     // its network's runs
        std::vector<UINT32> L, R;            // its junction stations towards the run before / after (global ids, junction list order)
        std::vector<UINT32> stations;        // L u R, ascending
        std::vector<UINT32> prev;            // stations of the running merged system ...
        ref prev_m;
        ref S;                               // ... and the last one: the run's system, its stations `stations`
    };
    struct span_t {
        int i = 0, j = 0;                    // its runs (indices into `runs`)
        int left = -1, right = -1, height = 0, depth = 0;
        std::vector<UINT32> stations;        // L(i) u R(j), ascending
        std::vector<UINT32> sys;             // global ids in the order of S's stations
        ref S;
    };

    const std::vector<blockMeta_t>& meta;
    const std::vector<block_t>& blocks;
    const std::vector<std::vector<UINT32>>& stn;
    lock_schedule_t& P;
    std::vector<run_t> runs;
    std::vector<span_t> spans;
    std::map<UINT32, std::array<double, 9>> end_con;       // constraint weights of the runs' end stations, by global id
    // the group being appended: one step of every run that has it, in batches of DNAGPU_CHAIN_BATCH_MAX (a run stays in the same
    // batch slot -- run / DNAGPU_CHAIN_BATCH_MAX -- through all groups: a slot's batches follow each other on one chain)
    lock_group_t group;
    UINT32 members = 0, slot = 0, block_steps = 0;
    double flops = 0.0, ref_flops = 0.0;

    // global ids of block k's kept stations at keep positions `pos` (all of them: nullptr)
    std::vector<UINT32> gids(UINT32 k, const std::vector<UINT32>* pos = nullptr) const {
        std::vector<UINT32> v;
        for (size_t p = 0; p < (pos ? pos->size() : blocks[k].keep.size()); ++p) v.push_back(stn[k][blocks[k].keep[pos ? (*pos)[p] : p]]);
        return v;
    }
    double nref3(UINT32 k) const {
        const double n = 3.0 * (double)stn[k].size();
        return n * n * n;
    }
    // constraint weights of end station s, at its position in `sorted`
    bool add_end_con(chain_step_data& d, const std::vector<UINT32>& sorted, UINT32 s) const {
        const auto it = end_con.find(s);
        const long q = position(sorted, s);
        if (it == end_con.end() || q < 0) return false;
        d.con_stn.push_back((UINT32)q);
        d.con_w9.insert(d.con_w9.end(), it->second.begin(), it->second.end());
        return true;
    }
    static int junction(const ref& r) { return r.kind == ref::jfwd || r.kind == ref::jrev ? 1 : 0; }

    void open_group() {
        group = {(UINT32)P.steps.batches(), 0};
        members = block_steps = 0;
        flops = ref_flops = 0.0;
    }
    // step d of `member` (a run, or a span's place in its level) with sources s0 (and s1) and output `out`
    void add(chain_step_data&& d, int member, ref s0, ref s1, ref out, double ref3 = 0.0) {
        if (members && (UINT32)(member / DNAGPU_CHAIN_BATCH_MAX) != slot) close_batch();
        slot = (UINT32)(member / DNAGPU_CHAIN_BATCH_MAX);
        d.n_src = s1.kind == ref::none ? 1 : 2;
        d.junction[0] = junction(s0);
        d.junction[1] = junction(s1);
        d.out_junction = junction(out);
        P.refs.push_back({s0, s1, out});
        flops += P.steps.add_step(std::move(d));
        ref_flops += ref3;
        block_steps += (UINT32)junction(out);       // (a step that leaves a junction matrix stands for a chain step on a block)
        ++members;
    }
    void close_batch() {
        P.steps.close_batch();
        P.batch_slot.push_back(slot);
    }
    void close_group(lock_lane_t& lane) {
        if (!members) return;
        close_batch();
        group.hi = (UINT32)P.steps.batches();
        lane.groups.push_back(group);
        lane.flops.push_back(flops);
        lane.ref_flops.push_back(ref_flops);
        lane.block_steps.push_back(block_steps);
    }
    lock_lane_t& new_stage(size_t lanes) {
        P.stages.emplace_back();
        P.stages.back().lanes.resize(lanes);
        return P.stages.back().lanes[0];
    }

    // the contiguous networks of the project (dnaadjust.cpp:10449-10474: a block whose junction list is empty ends one; an isolated block
    // is a network of its own without a chain step): their chains are independent of each other and advance together like the runs of one
    const char* choose_runs(int want) {
        struct net_t { UINT32 s, e; };
        std::vector<net_t> nets;
        const UINT32 B = (UINT32)blocks.size();
        UINT32 chained = 0;
        for (UINT32 k = 0, e; k < B; k = e + 1) {
            e = k;
            if (meta[k]._blockIsolated) continue;
            if (!meta[k]._blockFirst) return "a network that does not begin with a first block";
            while (!meta[e]._blockLast)
                if (++e >= B || meta[e]._blockIsolated || meta[e]._blockFirst) return "a network that does not end with a last block";
            if (e > k) nets.push_back({k, e});
            chained += e > k ? e - k + 1 : 0;
        }
        // (the runs' boundaries come from a scan -- level 2 below, 2 log2 W levels deep --, the steps inside the runs are 2 x blocks-per-run deep:
        //  about eight blocks to a run; dnasegment150's 666 blocks: 16 / 32 / 48 / 64 / 96 / 128 / 160 runs -> 47.0 / 38.0 / 35.7 / 34.3 / 34.0 / 34.4 / 36.0 ms)
        int W = want > 1 ? want : (chained >= 64 ? std::max<int>(16, std::min<int>(512, (int)(chained / 8))) : 1);
        W = std::min<int>(W, (int)(chained / 3));
        if (W < 2) return "too few chained blocks for two runs";
        // small condensed systems, every block between two others carrying something both ways
        for (const net_t& n : nets)
            for (UINT32 k = n.s; k <= n.e; ++k) {
                const block_t& Bk = blocks[k];
                if (Bk.keep.empty() || !Bk.red) return "a block without a condensed system";
                if (3 * Bk.keep.size() > 1024) return "a condensed block of more than 1024 unknowns";
                if ((k > n.s && Bk.c_prev.empty()) || (k < n.e && Bk.c_next.empty())) return "a block that shares no station with a neighbour";
                if ((k < n.e && !Bk.jfwd) || (k > n.s && !blocks[k - 1].jrev)) return "a junction matrix missing";
            }
        // the runs: W of them dealt to the networks by their length, at least three blocks to a run (two in a network of two blocks)
        for (const net_t& n : nets) {
            const UINT32 len = n.e - n.s + 1;
            const int nr = std::max(1, std::min<int>((int)(len / 3), (int)std::lround((double)W * len / (double)chained)));
            const int first = (int)runs.size();
            for (int i = 0; i < nr; ++i) {
                runs.push_back({n.s + (UINT32)((uint64_t)i * len / nr), n.s + (UINT32)((uint64_t)(i + 1) * len / nr) - 1, n.s, n.e, first, first + nr - 1});
                run_t& g = runs.back();
                if (g.a > g.s) g.L = gids(g.a, &blocks[g.a].c_prev);
                if (g.b < g.e) g.R = gids(g.b, &blocks[g.b].c_next);
                g.stations = sorted_union(g.L, g.R);
                for (const constraint_list block_t::*cl : {&block_t::ccon_fwd, &block_t::ccon_rev})
                    for (UINT32 k = g.a; k <= g.b; ++k) {
                        const constraint_list& src = blocks[k].*cl;
                        for (size_t q = 0; q < src.stn.size(); ++q) {
                            const UINT32 s = stn[k][blocks[k].keep[src.stn[q]]];
                            if (position(g.stations, s) >= 0) std::copy(src.w9.begin() + 9 * q, src.w9.begin() + 9 * q + 9, end_con[s].begin());
                        }
                    }
                g.prev = gids(g.a);
                g.prev_m = {ref::red, g.a};
            }
        }
        P.runs = (int)runs.size();
        return nullptr;
    }

    // level 1: the runs merged to their end stations, merge j of every run together
    const char* level1() {
        lock_lane_t& lane = new_stage(1);
        UINT32 longest = 0;
        for (const run_t& g : runs) longest = std::max(longest, g.b - g.a);
        for (UINT32 j = 1; j <= longest; ++j) {
            open_group();
            for (int r = 0; r < (int)runs.size(); ++r) {
                run_t& g = runs[r];
                if (g.b - g.a < j || g.first == g.last) continue;       // (a network that is one run needs no run system)
                const UINT32 k = g.a + j;
                chain_step_data d;
                const std::vector<UINT32> blk = gids(k), U = sorted_union(g.prev, blk);
                positions_in(U, g.prev, d.pos[0]);
                positions_in(U, blk, d.pos[1]);
                // stations that stay: the run's first junction row and block k's junction row towards k + 1
                const std::vector<UINT32> stay = sorted_union(g.L, k < g.e ? gids(k, &blocks[k].c_next) : std::vector<UINT32>{});
                if (!positions_in(U, stay, d.keep)) return "a merge inside a run that loses a junction station";
                // constraints of the stations that leave inside the run: where the forward chain adds them (first appearance)
                for (UINT32 kk : (k == g.a + 1 ? std::vector<UINT32>{g.a, k} : std::vector<UINT32>{k})) {
                    const constraint_list& src = blocks[kk].ccon_fwd;
                    for (size_t i = 0; i < src.stn.size(); ++i) {
                        const UINT32 s = stn[kk][blocks[kk].keep[src.stn[i]]];
                        if (position(g.stations, s) >= 0) continue;
                        d.con_stn.push_back((UINT32)position(U, s));
                        d.con_w9.insert(d.con_w9.end(), src.w9.begin() + 9 * i, src.w9.begin() + 9 * i + 9);
                    }
                }
                d.n_stn = (UINT32)U.size();
                const ref out{ref::merged, (UINT32)P.merged.size()};
                P.merged.push_back({(UINT32)stay.size(), k, "PrepareAdjustment(): run merge"});
                add(std::move(d), r, g.prev_m, {ref::red, k}, out);
                g.prev = stay;
                g.prev_m = out;
                if (k == g.b && stay != g.stations) return "a run whose last merge keeps other stations than its end stations";
                if (k == g.b) g.S = out;
            }
            close_group(lane);
        }
        return nullptr;
    }

    int build_span(int i, int j, int depth) {
        span_t sp;
        sp.i = i;
        sp.j = j;
        sp.depth = depth;
        sp.stations = sorted_union(runs[i].L, runs[j].R);
        if (i < j) {
            const int m = i + (j - i) / 2;
            sp.left = build_span(i, m, depth + 1);
            sp.right = build_span(m + 1, j, depth + 1);
            sp.height = 1 + std::max(spans[sp.left].height, spans[sp.right].height);
        } else {
            sp.S = runs[i].S;          // (a leaf's system is its run's)
            sp.sys = runs[i].stations;
        }
        spans.push_back(std::move(sp));
        return (int)spans.size() - 1;
    }

    // level 2: the junction matrices at the runs' boundaries -- forward (everything left of a boundary condensed onto it) and reverse -- as a
    // SCAN over the runs of a network instead of two chains of W - 1 steps each (round 6).  The runs' systems are the leaves of a binary
    // tree; going up, the two halves of a span are merged to the span's end stations (its first run's junction row towards the run
    // before, its last run's towards the run after: the step of level 1, on two systems); going down, a node hands the junction matrix
    // at its middle boundary to both sides -- forward from its left half and the forward matrix at its own left end, reverse from its
    // right half and the reverse matrix at its right end.  2 log2 W levels instead of W - 1, every level's steps of all networks in
    // merged launches; the same additions, associated differently: results agree with the step-by-step chains to rounding.
    // A station's constraint weights go in where the station leaves (a merge) or where the chain in question meets it first (a
    // boundary step: the stations that stay, unless the matrix carried in has them already) -- once per direction, as in
    // AddConstraintStationstoNormalsForward / ...Reverse (ADJ:1884-1958).
    const char* level2() {
        for (size_t r = 0; r < runs.size(); r = runs[r].last + 1)
            if (runs[r].last > runs[r].first) build_span(runs[r].first, runs[r].last, 0);
        int top = 0, deepest = 0;
        for (const span_t& sp : spans) {
            top = std::max(top, sp.height);
            deepest = std::max(deepest, sp.depth);
        }
        const char* lost = "a step of the scan over the runs that loses a station";
        // ... going up: the spans that somebody's boundary step needs (all but the roots), lowest first.  (One lane beside an empty one:
        // a stage of ONE lane has its batches dealt to the chains, and a merge reads what any batch of the level below has written.)
        lock_lane_t& up = new_stage(2);
        for (int h = 1; h < top; ++h) {
            open_group();
            int idx = 0;
            for (span_t& N : spans) {
                if (N.height != h || N.depth == 0) continue;
                const span_t &A = spans[N.left], &Bs = spans[N.right];
                chain_step_data d;
                const std::vector<UINT32> U = sorted_union(A.stations, Bs.stations);
                if (!positions_in(U, A.sys, d.pos[0]) || !positions_in(U, Bs.sys, d.pos[1]) || !positions_in(U, N.stations, d.keep)) return lost;
                for (UINT32 s : U)
                    if (position(N.stations, s) < 0 && !add_end_con(d, U, s)) return lost;
                d.n_stn = (UINT32)U.size();
                N.S = {ref::merged, (UINT32)P.merged.size()};
                N.sys = N.stations;
                P.merged.push_back({(UINT32)N.stations.size(), runs[N.i].a, "PrepareAdjustment(): span merge"});
                add(std::move(d), idx++, A.S, Bs.S, N.S);
            }
            close_group(up);
        }
        // ... going down: the node's middle boundary, forward (lane 0) and reverse (lane 1)
        lock_lane_t* down = &new_stage(2);
        for (int dir = 0; dir < 2; ++dir)
            for (int dep = 0; dep <= deepest; ++dep) {
                open_group();
                int idx = 0;
                for (const span_t& N : spans) {
                    if (N.depth != dep || N.left < 0) continue;
                    const int m = spans[N.left].j;          // the boundary between runs m and m + 1
                    const span_t& H = spans[dir == 0 ? N.left : N.right];      // the half the boundary's matrix is condensed from
                    const std::vector<UINT32>&Lh = runs[H.i].L, &Rh = runs[H.j].R;
                    const std::vector<UINT32>& in = dir == 0 ? Lh : Rh;       // where the carried matrix comes in (none at the network's end) ...
                    const std::vector<UINT32>& outl = dir == 0 ? Rh : Lh;     // ... and what this step leaves
                    chain_step_data d;
                    if (!positions_in(H.stations, H.sys, d.pos[0]) || !positions_in(H.stations, outl, d.keep) || !positions_in(H.stations, in, d.pos[1]))
                        return lost;
                    const std::set<UINT32> in_set(in.begin(), in.end()), from_left(Lh.begin(), Lh.end());
                    for (UINT32 s : outl)
                        if (!in_set.count(s) && !add_end_con(d, H.stations, s)) return lost;
                    for (UINT32 s : H.stations) {
                        const UINT32 k = from_left.count(s) ? runs[H.i].a : runs[H.j].b;
                        const long q = position(stn[k], s);
                        if (q < 0) return lost;
                        d.est_blk.push_back(k);
                        d.est_idx.push_back((UINT32)q);
                    }
                    d.n_stn = (UINT32)H.stations.size();
                    const ref carried = dir == 0 ? (H.i > runs[H.i].first ? ref{ref::jfwd, runs[H.i].a - 1} : ref{})
                                                 : (H.j < runs[H.j].last ? ref{ref::jrev, runs[H.j].b} : ref{});
                    // (what the chain's step on that block leaves: counted as that step)
                    add(std::move(d), idx++, H.S, carried, dir == 0 ? ref{ref::jfwd, runs[m].b} : ref{ref::jrev, runs[m + 1].a - 1},
                        nref3(dir == 0 ? runs[m].b : runs[m + 1].a));
                }
                close_group(down[dir]);
            }
        return nullptr;
    }

    // level 3: both chains inside every run, from the boundary values of level 2 (CondensedForwardBlock / CondensedReverseBlock as data)
    // (a lane per direction and batch slot: the slots of a direction are independent of each other and go to chains of their own)
    void level3() {
        const int W = (int)runs.size(), slots = (W + DNAGPU_CHAIN_BATCH_MAX - 1) / DNAGPU_CHAIN_BATCH_MAX;
        UINT32 longest = 0;
        for (const run_t& g : runs) longest = std::max(longest, g.b - g.a);
        lock_lane_t* lanes = &new_stage((size_t)(2 * slots));
        for (int sl = 0; sl < slots; ++sl)
            for (int dir = 0; dir < 2; ++dir)
                for (UINT32 j = 0; j <= longest; ++j) {
                    open_group();
                    for (int r = sl * DNAGPU_CHAIN_BATCH_MAX; r < std::min(W, (sl + 1) * DNAGPU_CHAIN_BATCH_MAX); ++r) {
                        const run_t& g = runs[r];
                        if (g.a + j + 1 > g.b) continue;
                        const UINT32 k = dir == 0 ? g.a + j : g.b - j;
                        const block_t& Bk = blocks[k];
                        chain_step_data d;
                        d.n_stn = (UINT32)Bk.keep.size();
                        d.est_blk.assign(Bk.keep.size(), k);
                        d.est_idx = Bk.keep;
                        d.pos[0].resize(Bk.keep.size());
                        std::iota(d.pos[0].begin(), d.pos[0].end(), 0u);
                        const constraint_list& con = dir == 0 ? Bk.ccon_fwd : Bk.ccon_rev;
                        d.con_stn = con.stn;
                        d.con_w9 = con.w9;
                        d.keep = dir == 0 ? Bk.c_next : Bk.c_prev;
                        const bool carried = dir == 0 ? k > g.s : k < g.e;
                        if (carried) d.pos[1] = dir == 0 ? Bk.c_prev : Bk.c_next;
                        const ref in = !carried ? ref{} : dir == 0 ? ref{ref::jfwd, k - 1} : ref{ref::jrev, k};
                        add(std::move(d), r, {ref::red, k}, in, dir == 0 ? ref{ref::jfwd, k} : ref{ref::jrev, k - 1}, nref3(k));
                    }
                    close_group(lanes[2 * sl + dir]);
                }
    }
};

const char* dna_adjust::ScheduleLockstepChains(const std::vector<blockMeta_t>& meta, const std::vector<block_t>& blocks,
                                               const std::vector<std::vector<UINT32>>& stations, int want, lock_schedule_t& out) {
    out = lock_schedule_t();
    lock_scheduler s{meta, blocks, stations, out};
    const char* why = s.choose_runs(want);
    if (!why) why = s.level1();
    if (!why) why = s.level2();
    if (!why) s.level3();
    return why;
}

}  // namespace networkadjust
}  // namespace dynadjust
