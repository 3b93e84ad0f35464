// kanpyo_amd/csrc/kgpu_lock.h -- SpinLock, the small-call combiner's lock (kgpu_small.cpp), on its own: tests/c_abi/lock_stress.cpp includes it too.
#pragma once
#include <atomic>
#include <cstdint>
#include <sched.h>
#include <linux/futex.h>
#include <sys/syscall.h>
#include <unistd.h>

// The combiner's lock: held for a push_back and two additions (tens of nanoseconds), taken by every caller -- and by a whole batch's followers at the same
// instant, when the leader's one wake-up releases them into their next calls.  A pthread mutex puts each of them to sleep and wakes it again through the kernel:
// measured with 128 callers, 40-48 us of (system) CPU per call in the lock alone -- more CPU than a 16-CPU cgroup quota grants, so the group spent most of each
// 100 ms period throttled (profiles/experiments/r05_callers_cpu.txt).  Test-and-test-and-set with pause and backoff, a few yields, then asleep on the word.
struct SpinLock {
    // 0 free, 1 held, 2 held and somebody may be asleep on the word.  Spinning is bounded (round 6, advisor): a holder that lost its CPU -- more callers than
    // CPUs, a cgroup quota, a lower-priority holder under SCHED_FIFO -- is not waited for with yields for ever; after ~four yields the waiter sleeps on the
    // word (futex) and the release wakes one sleeper.  The uncontended and the briefly contended paths never enter the kernel.
    std::atomic<uint32_t> v{0};
    void lock() {
        // (a lost compare-and-swap backs off for twice as long, up to 32 pauses: two dozen threads that all saw the word free do not all write it again at the next release)
        for (unsigned spins = 0, backoff = 1, yields = 0; yields < 4;) {
            if (v.load(std::memory_order_relaxed) == 0) {
                uint32_t z = 0;
                if (v.compare_exchange_weak(z, 1, std::memory_order_acquire, std::memory_order_relaxed)) return;
                for (unsigned k = 0; k < backoff; ++k) cpu_relax();
                if (backoff < 32) backoff *= 2;
            }
            cpu_relax();
            if (++spins >= 2048) { sched_yield(); spins = 0; ++yields; }
        }
        while (v.exchange(2, std::memory_order_acquire) != 0) syscall(SYS_futex, (uint32_t *)&v, FUTEX_WAIT_PRIVATE, 2u, nullptr, nullptr, 0);
    }
    void unlock() {
        if (v.exchange(0, std::memory_order_release) == 2) syscall(SYS_futex, (uint32_t *)&v, FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
    }
    static void cpu_relax() {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
};
