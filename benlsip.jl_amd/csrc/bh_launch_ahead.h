// The launch-ahead schedule of the host loops (pcg_run and cauchy_impl in bh_api.hip): how many launch units the host enqueues before
// it looks at the progress word, and what it may conclude from the word.  Plain values and two callables (no HIP type, no library
// state), so that the host compiler can build it into a test program (tests/test_launch_ahead_cpu.py).
//
// A launch unit is what one iteration (CG) or one pass (Cauchy search) enqueues.  Units enqueued past the end of the device-side loop
// are gated no-ops — cheap (~1.5 us per kernel) but not free, and over RCCL each still pays for its collective.  So: first a batch
// sized by what is known about the call (launch_ahead_first), then, while the loop is still running, launch-ahead batches: batch k+1
// is enqueued before the host looks at the state batch k left, so the GPU never waits for the host.
//
// THE LOCK-STEP RULE.  With several ranks every unit holds a collective, so every rank must take the SAME launch decisions.  The
// progress word keeps advancing while launch-ahead batches run, and ranks poll it at different moments: a decision taken after
// waiting for `target` units may therefore use only "the loop had ended by unit `target`" (done && n_hmul <= target) — never a
// later state that one rank happened to see.  lock_step = true holds a loop to that rule; lock_step = false (one rank, or an
// exchange inside a kernel that gated launches skip) decides on `done` as seen.
#pragma once
#include <algorithm>

namespace bh {

// The host-mapped progress word [tag | status | done | iter | n_hmul], unpacked (wait_mirror in bh_api.hip).
struct MirrorWord { int done, status, iter, n_hmul; };

constexpr int kFirstBatchCap = 32;
constexpr int kLaunchAheadNever = 0x7fffffff;      // an n_hmul target no word reaches

// The first batch of a CG loop is sized by the previous call on the handle (consecutive subproblems of a minor loop behave alike):
// an exact prediction means no gated launches and no host round trip inside the loop at all.  cold: without history.
inline int launch_ahead_first(int last_n_hmul, int cold) { return last_n_hmul > 0 ? std::min(last_n_hmul, kFirstBatchCap) : cold; }

struct LaunchAhead {
    int max_units;       // the loop cannot take more units than this (off included)
    int first;           // units of the first batch
    int batch;           // units of every later batch
    int off;             // unit k carries the decision of unit k - off (the one-kernel Cauchy pass: 1): u units stand for u - off products
    bool await_iter;     // progress is awaited on `iter` reaching target + 1 (the unit behind the target speaks for it), else on n_hmul >= target
    bool lock_step;      // decisions follow the lock-step rule above
    bool look_first;     // the host looks at the word behind the first batch; false: one batch more goes out first
};

// enqueue(i): enqueue launch unit i (0-based), 0 on success.  wait(n_hmul_target, iter_target, &word): block until the word shows
// `done`, n_hmul >= n_hmul_target, or (iter_target > 0) iter >= iter_target; 0 on success.  Returns the first non-zero code of
// either, else 0 with the final word in *mw (everything enqueued has spoken, or `done`).
template <class Enqueue, class Wait>
int launch_ahead(const LaunchAhead& s, Enqueue&& enqueue, Wait&& wait, MirrorWord* mw) {
    int launched = 0;
    auto launch_batch = [&](int nb) -> int {
        nb = std::min(nb, s.max_units - launched);
        for (int i = 0; i < nb; ++i, ++launched)
            if (const int rc = enqueue(launched)) return rc;
        return 0;
    };
    auto await = [&](int target) -> int {
        return s.await_iter ? wait(kLaunchAheadNever, target + 1, mw) : wait(target, 0, mw);
    };
    auto ended = [&](int target) { return mw->done && (!s.lock_step || mw->n_hmul <= target); };
    *mw = MirrorWord{};
    int rc = launch_batch(s.first);
    bool running = true;
    if (rc == 0 && s.look_first) {
        rc = await(launched - s.off);
        running = rc == 0 && !ended(launched - s.off) && launched < s.max_units;
        if (running) rc = launch_batch(s.batch);
    }
    while (rc == 0 && running) {
        const int target = launched - s.off;           // everything enqueued so far except the batch launched next
        const bool more = launched < s.max_units;
        if (more && (rc = launch_batch(s.batch))) break;
        if ((rc = await(target))) break;
        running = !ended(target) && more;
    }
    if (rc) return rc;
    return s.await_iter ? wait(kLaunchAheadNever, 0, mw) : wait(launched - s.off, 0, mw);
}

}  // namespace bh
