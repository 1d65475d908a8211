// The cycle hand-offs (csrc/sns_policy.h: policy::Handoff, policy::first_sweep_owner) on their own, for tests/test_host.py.
// argv[1] holds the raw sns_options; stdin one request per line, stdout one line per request:
//   E <events>   the events as given: B begin_solve | K v c krylov_did_first_sweep | O promise_operator | N l enter_level |
//                C l v put_carried | T l v take_put | A rc v end_pc_apply.  Levels are integers, vectors small integer names.
//   S nranks rep_level fuse_puts krylov method empty_from solves nl rows[nl]
//                the events a solve of the library emits on the plan policy::plan_cycle makes of a hierarchy of that shape (the
//                facts of sns_host_cycle_policy: every level window-capable, M = A P everywhere); see `Solve` below
//   W nranks rep_level nl rows[nl]
//                policy::first_sweep_owner of every level of that plan, with the plan's fuses_next_first column and
//                rep_gather_first
// Every event prints as <letter><args>=<legal>[/<answer>]; A appends the state it leaves: /<level of put outstanding>/<vector>.
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "sns_policy.h"

using namespace sns::policy;

static char names[4096];                                     // a vector's name n is the address &names[n]: compared, never read
static const void* vec(int n) { return &names[(unsigned)n % sizeof(names)]; }
static int name_of(const void* v) { return v ? (int)((const char*)v - names) : -1; }

struct Recorder {                                            // every transition, printed as it is made
    Handoff H;
    std::string out;
    void say(const char* fmt, int a = 0, int b = 0, int c = 0, int d = 0, int e = 0) {
        char buf[96];
        std::snprintf(buf, sizeof(buf), fmt, a, b, c, d, e);
        out += buf;
    }
    bool begin() { const bool ok = H.begin_solve(); say("B=%d ", ok); return ok; }
    bool krylov(int v, bool carried) { const bool ok = H.krylov_did_first_sweep(vec(v), carried); say("K%d.%d=%d ", v, carried, ok); return ok; }
    void promise() { H.promise_operator(); say("O "); }
    bool enter(int l) { const bool a = H.enter_level(l); say("N%d=1/%d ", l, a); return a; }
    bool carried(int l, int v) { const bool ok = H.put_carried(l, vec(v)); say("C%d.%d=%d ", l, v, ok); return ok; }
    bool take(int l, int v) { bool done = false; const bool ok = H.take_put(l, vec(v), &done); say("T%d.%d=%d/%d ", l, v, ok, done); return ok; }
    bool end(bool ok_call, int z) {
        const bool ok = H.end_pc_apply(ok_call, vec(z));
        say("A%d.%d=%d/%d/%d ", ok_call ? 0 : -1, z, ok, H.outstanding(), name_of(H.put.empty() ? nullptr : H.put[0]));
        return ok;
    }
};

// ---- TRANSCRIPTION (events only) of the library's call order: bicg_update / the Krylov methods (csrc/sns_krylov.hip) -> pc_apply ->
// vcycle / vcycle_windows (csrc/sns_cycle.hip) -> exchange_and_spmv (csrc/sns_ctx.h).  Kept in step with them by hand: where they
// make a transition of the hand-off state, this makes the same one, under the same conditions of the plan and of the rank
// (`rows`: the rank has rows on the level; a PutDst is taken to be available wherever the library asks the plan for one).
struct Solve {
    CyclePlan plan;
    int nranks = 1, R = 0, empty_from = 99;
    Recorder rec;
    enum { X_KRYLOV = 1, PH = 2, SH = 3, TMP = 4, ZJ = 5, REP_X = 90 };
    int X(int l) const { return 100 + 2 * l; }
    int pong(int l) const { return 101 + 2 * l; }
    bool rows(int l) const { return l < empty_from || (R > 0 && l >= R); }
    int start(int l, int x) const { return name_of(cycle_start(plan.level[(size_t)l], vec(x), vec(pong(l)))); }
    int fine_vector(int z) const { return (nranks > 1 && !plan.fine_tails_unused) ? X(0) : z; }
    FirstSweepOwner owner(int l) const { return first_sweep_owner(plan, R, l); }

    bool cycle_windows(int l, int x) {
        const LevelPlan& Q = plan.level[(size_t)l];
        const LevelPlan& QC = plan.level[(size_t)l + 1];
        int cur = start(l, x), oth = cur == x ? pong(l) : x;
        const bool pdl = plan.fuse_puts && Q.blocks && rows(l);
        auto carry = [&](bool pd, int lv, int v) { return !pd || rec.carried(lv, v); };
        const bool by_krylov = rec.enter(l);
        if (!by_krylov && rows(l) && owner(l) == FIRST_SWEEP_LEVEL && !carry(pdl, l, cur)) return false;
        for (int s = 1; s < Q.pre; ++s) {
            if (!rec.take(l, cur)) return false;
            if (rows(l) && Q.blocks && !carry(pdl, l, oth)) return false;
            std::swap(cur, oth);
        }
        const bool rep_src = R > 0 && l + 1 == R - 1;
        const int cx = rep_src ? (int)REP_X : X(l + 1);
        if (!rec.take(l, cur)) return false;
        const bool pdc = plan.fuse_puts && owner(l + 1) == FIRST_SWEEP_RESTRICTION && QC.blocks && !rep_src && QC.windows &&
                         rows(l + 1) && (l == 0 || rows(l));
        if (!carry(pdc, l + 1, start(l + 1, X(l + 1)))) return false;
        if (!cycle(l + 1, rep_src ? -1 : X(l + 1))) return false;
        if (!(rep_src && l >= 1) && !rec.take(l + 1, cx)) return false;
        const bool last_puts = pdl && (l == 0 ? rec.H.op_promised : plan.level[(size_t)l - 1].windows != 0);
        if (rows(l) && !carry((Q.post > 1 || last_puts) && pdl, l, oth)) return false;
        std::swap(cur, oth);
        for (int s = 1; s < Q.post; ++s) {
            if (!rec.take(l, cur)) return false;
            if (rows(l) && Q.blocks && !carry((s + 1 < Q.post || last_puts) && pdl, l, oth)) return false;
            std::swap(cur, oth);
        }
        return cur == x;
    }
    bool cycle(int l, int x) {
        const int nl = (int)plan.level.size();
        if (R > 0 && l == R - 1) return cycle(R, X(R));      // enter_replicated_tail
        if (l + 1 == nl) return true;                        // solve_last_level
        if (plan.level[(size_t)l].windows) return cycle_windows(l, x);
        rec.enter(l);                                        // (the exchange form: nothing else is handed over)
        return cycle(l + 1, (R > 0 && l + 1 == R - 1) ? -1 : X(l + 1));
    }
    bool pc_apply(int z) {
        const bool ok = cycle(0, fine_vector(z));
        return rec.end(ok, z) && ok;
    }
    bool op_apply(int x) { return !plan.fine_windows || rec.take(0, x); }     // exchange_and_spmv, the window branch
    bool bicg_update(bool krylov, int z) {
        const LevelPlan& P = plan.level[0];
        if (!krylov || owner(0) != FIRST_SWEEP_LEVEL || P.lp_fmt == 0 || !rows(0)) return true;
        return rec.krylov(start(0, fine_vector(z)), P.blocks && plan.fuse_puts && P.windows);
    }
    bool solve(int method, bool krylov) {
        if (!rec.begin() || !op_apply(X_KRYLOV)) return false;
        if (method == 0) {                                   // bicgstab: first_half | [update, pc, op | update, first_half]*
            auto first_half = [&]() { rec.promise(); return pc_apply(PH) && op_apply(PH); };
            if (!first_half()) return false;
            for (int it = 0; it < 2; ++it) {
                if (!bicg_update(krylov, SH)) return false;
                rec.promise();
                if (!pc_apply(SH) || !op_apply(SH)) return false;
                if (it == 0 && (!bicg_update(krylov, PH) || !first_half())) return false;
            }
        } else if (method == 1) {                            // fgmres: [pc, op]*
            for (int j = 0; j < 2; ++j)
                if (!pc_apply(ZJ + j) || !op_apply(ZJ + j)) return false;
        } else {                                             // tfqmr: [pc, op]*, then a pc_apply no operator follows
            for (int j = 0; j < 3; ++j)
                if (!pc_apply(TMP) || !op_apply(TMP)) return false;
            if (!pc_apply(TMP)) return false;
        }
        return op_apply(X_KRYLOV);
    }
};
// ---- end of the transcription

static bool plan_of(std::istringstream& in, const sns_options& o, int nranks, int R, bool fuse_puts, CyclePlan& p) {
    int nl = 0;
    if (!(in >> nl) || nl < 1 || nl > 16 || R < 0 || R >= nl || R == 1 || nranks < 1) return false;
    Facts f;
    f.nranks = nranks;
    f.rep_level = R;
    for (int l = 0; l < nl; ++l) { long long r = 0; if (!(in >> r)) return false; f.rows.push_back(r); }
    f.max_owned.assign((size_t)nl, 0);
    f.has_blocks.assign((size_t)nl, 1);
    f.has_ap.assign((size_t)nl, 1);
    f.has_ap_rep.assign((size_t)nl, 1);
    f.win_capable.assign((size_t)nl, 1);
    f.rows_global_l1 = nl > 1 ? f.rows[1] : 0;
    f.windows = true;
    f.rep_gather_fits = true;
    f.last = coarsest_kind(o, f.rows[(size_t)nl - 1]);
    f.fuse_puts = fuse_puts;
    p = plan_cycle(o, f);
    return true;
}

int main(int argc, char** argv) {
    sns_options o;
    FILE* fo = argc > 1 ? std::fopen(argv[1], "rb") : nullptr;
    if (!fo || std::fread(&o, sizeof(o), 1, fo) != 1) return 2;
    std::fclose(fo);
    char line[4096];
    while (std::fgets(line, sizeof(line), stdin)) {
        std::istringstream in(line);
        std::string what;
        if (!(in >> what)) continue;
        if (what == "E") {
            Recorder rec;
            std::string ev;
            int a = 0, b = 0;
            bool bad = false;
            while (!bad && in >> ev) {
                if (ev == "B") rec.begin();
                else if (ev == "O") rec.promise();
                else if (ev == "N" && in >> a) rec.enter(a);
                else if (ev == "K" && in >> a >> b) rec.krylov(a, b != 0);
                else if (ev == "C" && in >> a >> b) rec.carried(a, b);
                else if (ev == "T" && in >> a >> b) rec.take(a, b);
                else if (ev == "A" && in >> a >> b) rec.end(a == 0, b);
                else bad = true;
            }
            if (bad) return 3;
            std::printf("%s\n", rec.out.c_str());
        } else if (what == "S") {
            Solve s;
            int fuse = 1, krylov = 0, method = 0, solves = 1;
            if (!(in >> s.nranks >> s.R >> fuse >> krylov >> method >> s.empty_from >> solves)) return 3;
            if (!plan_of(in, o, s.nranks, s.R, fuse != 0, s.plan)) return 4;
            std::printf("P %d %d %d %d", s.plan.fine_windows, s.plan.fine_tails_unused, s.plan.rep_gather_first, s.plan.fuse_puts);
            for (const LevelPlan& q : s.plan.level)
                std::printf(" ; %d %d %d %d %d %d", q.cycled ? q.kind : -1, q.cycled ? q.pre : 0, q.cycled ? q.post : 0, q.exact, q.windows, q.blocks);
            bool ok = true;
            for (int k = 0; k < solves && ok; ++k) ok = s.solve(method, krylov != 0);
            std::printf(" | %d | %s\n", ok, s.rec.out.c_str());
        } else if (what == "W") {
            CyclePlan p;
            int nranks = 1, R = 0;
            if (!(in >> nranks >> R) || !plan_of(in, o, nranks, R, true, p)) return 4;
            std::printf("%d", p.rep_gather_first);
            for (int l = 0; l < (int)p.level.size(); ++l) std::printf(" %d:%d", p.level[(size_t)l].fuses_next_first, (int)first_sweep_owner(p, R, l));
            std::printf(" %d\n", (int)first_sweep_owner(p, R, (int)p.level.size()));
        } else {
            return 3;
        }
    }
    return 0;
}
