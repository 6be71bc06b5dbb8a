// amg_cycle_check.cpp -- the host-pure order of a multigrid cycle and the rule of the fused tail (csrc/spk_host.cpp:
// amg_cycle_steps, amg_tail_first, amg_tail_runs) at L = 1, 2 and 16, and where the iterate of each level lies after each
// step (amg_cycle_buffers) at L = 2, 3 and 5, without a GPU: compiled with g++ and the sanitizers by
// tests/test_mg_cycle_cpu.py.
#include <cstdio>
#include <vector>

#include "spk_host.hpp"

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);  \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

using spk::AmgStep;

// the definition again, as a loop over an explicit stack of (level, fresh, stage)
static std::vector<AmgStep> steps_ref(int L, bool w)
{
    struct Frame { int l; bool fresh; int stage; };
    std::vector<AmgStep> out;
    std::vector<Frame> st{{0, true, 0}};
    while (!st.empty()) {
        Frame &f = st.back();
        if (f.l == L - 1) { out.push_back({SPK_AMG_STEP_COARSE, f.l}); st.pop_back(); continue; }
        const int l = f.l;
        if (f.stage == 0) {
            out.push_back({f.fresh ? SPK_AMG_STEP_PRE0 : SPK_AMG_STEP_PRE, l});
            out.push_back({SPK_AMG_STEP_DOWN, l});
            f.stage = 1;
            st.push_back({l + 1, true, 0});
        } else if (f.stage == 1 && w && l + 1 < L - 1) {
            f.stage = 2;
            st.push_back({l + 1, false, 0});
        } else {
            out.push_back({SPK_AMG_STEP_UP, l});
            out.push_back({SPK_AMG_STEP_POST, l});
            st.pop_back();
        }
    }
    return out;
}

static bool same(const std::vector<AmgStep> &a, const std::vector<AmgStep> &b)
{
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i)
        if (a[i].kind != b[i].kind || a[i].level != b[i].level) return false;
    return true;
}

// amg_cycle_buffers against the launches' rule, walked step by step as smooth() and amg_apply (spk_amg_cycle.cpp) walk
// it: cur[l] is the buffer (0: ya, 1: yb) that holds the iterate of level l, -1 while it has none.  Each single smoothing
// step writes the buffer its input is not in, a fresh start writes ya, the coarse solve writes ya, UP works in place.
// The fields are compared where the tail kernel reads them: sel at PRE, POST, DOWN and UP, sel_next at UP.
static void check_buffers(int L, int cycle, int nu, int t)
{
    const std::vector<AmgStep> st = spk::amg_cycle_steps(L, cycle);
    const auto runs = spk::amg_tail_runs(st, t);
    const spk::AmgBuffers b = spk::amg_cycle_buffers(st, runs, L, nu, t);
    CHECK(b.sel.size() == st.size() && b.sel_next.size() == st.size() && b.run_sel.size() == runs.size());
    CHECK(!runs.empty());
    std::vector<int> cur((size_t)L, -1);
    size_t run = 0;
    for (size_t i = 0; i < st.size(); ++i) {
        const size_t l = (size_t)st[i].level;
        switch (st[i].kind) {
        case SPK_AMG_STEP_PRE0: cur[l] = -1;   // the zero guess: no input buffer
            [[fallthrough]];
        case SPK_AMG_STEP_PRE:
        case SPK_AMG_STEP_POST:
            if (st[i].kind != SPK_AMG_STEP_PRE0) CHECK(cur[l] >= 0 && b.sel[i] == cur[l]);
            for (int k = 0; k < nu; ++k) cur[l] = cur[l] == 0 ? 1 : 0;   // dst = y == ya ? yb : ya
            break;
        case SPK_AMG_STEP_DOWN: CHECK(cur[l] >= 0 && b.sel[i] == cur[l]); break;
        case SPK_AMG_STEP_COARSE: cur[l] = 0; break;
        default:   // SPK_AMG_STEP_UP
            CHECK(cur[l] >= 0 && b.sel[i] == cur[l]);
            CHECK(cur[l + 1] >= 0 && b.sel_next[i] == cur[l + 1]);
        }
        if (run < runs.size() && (size_t)runs[run].second == i + 1) {
            CHECK(cur[(size_t)t] >= 0 && b.run_sel[run] == cur[(size_t)t]);
            ++run;
        }
    }
    CHECK(run == runs.size());
}

int main()
{
    for (int L : {2, 3, 5})
        for (int cycle : {SPK_AMG_CYCLE_V, SPK_AMG_CYCLE_W})
            for (int nu : {1, 2, 3})
                for (int t : {1, 2, L - 1})
                    if (t >= 1 && t <= L - 1) check_buffers(L, cycle, nu, t);
    for (int L : {1, 2, 16})
        for (int cycle : {SPK_AMG_CYCLE_V, SPK_AMG_CYCLE_W}) {
            const bool w = cycle == SPK_AMG_CYCLE_W;
            const std::vector<AmgStep> st = spk::amg_cycle_steps(L, cycle);
            CHECK(same(st, steps_ref(L, w)));
            // entries per level: a level is entered at its PRE0 / PRE, the coarsest at its COARSE
            std::vector<long> entered((size_t)L, 0);
            for (const AmgStep &s : st)
                if (s.kind == SPK_AMG_STEP_PRE0 || s.kind == SPK_AMG_STEP_PRE || s.kind == SPK_AMG_STEP_COARSE) ++entered[(size_t)s.level];
            for (int l = 0; l < L; ++l) {
                const long want = !w ? 1 : l < L - 1 ? 1l << l : L >= 2 ? 1l << (L - 2) : 1;
                CHECK(entered[(size_t)l] == want);
            }
            // the tail rule on rows 2^(L-l) * 3: every level's size, one less, and 1
            std::vector<int32_t> rows((size_t)L);
            for (int l = 0; l < L; ++l) rows[(size_t)l] = 3 << (L - l);
            CHECK(spk::amg_tail_first(L, rows.data(), cycle, SPK_AMG_TAIL_LAUNCHES, rows[(size_t)L - 1]) == -1);
            CHECK(spk::amg_tail_runs(st, -1).empty());
            for (int l = 0; l < L; ++l) {
                const int t = spk::amg_tail_first(L, rows.data(), cycle, SPK_AMG_TAIL_FUSED, rows[(size_t)l]);
                CHECK(t == (L < 2 ? -1 : l == 0 ? 1 : l));   // level 0 is never in the tail
                const int t1 = spk::amg_tail_first(L, rows.data(), cycle, SPK_AMG_TAIL_FUSED, rows[(size_t)l] - 1);
                CHECK(t1 == (l + 1 < L ? l + 1 : -1));
                if (t < 1) continue;
                const auto runs = spk::amg_tail_runs(st, t);
                const long want = !w ? 1 : t < L - 1 ? 1l << (t - 1) : 1l << (L - 2);
                CHECK((long)runs.size() == want);
                long covered = 0, in_tail = 0;
                for (const auto &r : runs) {
                    CHECK(r.first < r.second);
                    CHECK(r.first == 0 || st[(size_t)r.first - 1].level < t);                    // maximal
                    CHECK((size_t)r.second == st.size() || st[(size_t)r.second].level < t);
                    for (int64_t i = r.first; i < r.second; ++i) CHECK(st[(size_t)i].level >= t);
                    covered += (long)(r.second - r.first);
                }
                for (const AmgStep &s : st) in_tail += s.level >= t;
                CHECK(covered == in_tail);
            }
            CHECK(spk::amg_tail_first(L, rows.data(), cycle, SPK_AMG_TAIL_FUSED, 1) == -1);
            CHECK(spk::amg_tail_first(L, rows.data(), cycle, SPK_AMG_TAIL_AUTO, rows[0]) == (w && L >= 2 ? 1 : -1));
        }
    for (int bad : {0, SPK_AMG_MAX_LEVELS + 1}) {
        bool threw = false;
        try { spk::amg_cycle_steps(bad, SPK_AMG_CYCLE_V); } catch (const spk::Error &e) { threw = e.code == SPK_ERR_ARG; }
        CHECK(threw);
    }
    if (failures) return 1;
    std::printf("all multigrid cycle host checks passed\n");
    return 0;
}
