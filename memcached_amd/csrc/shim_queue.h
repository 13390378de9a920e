// shim_queue.h -- the coalescing queue of crc32c_batch_submit / _wait and
// crc32c_batch_multi's persistent per-device workers.
#pragma once

// The read-verify CRCs arrive from many IO threads, each with a batch of at
// most io_depth reads (extstore.c:853-945; io_depth = 1 by default,
// storage.c:1339).  One synchronous GPU call per such batch costs a launch and
// a round trip per thread; the queue instead lets every thread enqueue its
// spans and a per-device dispatcher packs whatever is pending into one k_small
// launch, reading the spans where they lie in page-locked host memory
// (group commit: while one launch runs, the next batch accumulates).
struct crc32c_job {
    crc32c_spans s;
    unsigned flags = 0;
    // CRC32C_DEVICE jobs: recorded on the submitter's default stream, waited
    // for by the queue's stream before the job runs (work the caller queued on
    // the default stream, e.g. the copy filling the spans, stays ordered first)
    hipEvent_t after = nullptr;
    const uint8_t *dbase = nullptr;  // coalesced jobs: the device view of s.base
    // pointer jobs (crc32c_ptrs_submit): the caller's batch -- s holds its
    // lens, len, crc_in, out and n, what launch and finish read of any job --
    // and each span's device view, translated at submit time (empty: a device
    // job, or some span is pageable)
    bool ptr = false;
    crc32c_ptr_batch pb{};
    std::vector<const uint8_t *> views;
    bool coalesce = false;
    int rc = CRC32C_OK;
    std::atomic<int> done{0};
    Queue *q = nullptr;
};

namespace {

constexpr uint64_t kQueueSpanMax = 256u << 10;  // longer spans: the job runs alone (planned path)
int run_ptr_job(Device &d, crc32c_job *j, hipStream_t st);  // shim_ptrs.h

static_assert(sizeof(std::atomic<int>) == sizeof(int) && std::atomic<int>::is_always_lock_free,
              "crc32c_job::done is waited on as a futex word");

struct Queue {
    Device *d = nullptr;
    std::mutex mu;
    std::condition_variable cv_work;
    std::deque<crc32c_job *> pending;
    hipStream_t st = nullptr;
    // Two launch slots: while one launch runs, the next (whatever was pending
    // when it started) is queued behind it on the stream.  Each slot has
    // pinned, mapped descriptors for kSmallMax spans and its event.
    struct Slot {
        MapBuf<uint64_t> addr;
        MapBuf<uint32_t> len, cin, out;
        hipEvent_t done = nullptr;
        std::vector<crc32c_job *> jobs;  // empty: the slot is free
    } slot[2];
    unsigned long long *dnbad = nullptr;  // (spans are absolute: never out of range)
    std::atomic<uint64_t> launches{0}, spans{0}, jobs{0}, solo{0};

    int init(Device &dev) {
        d = &dev;
        HIP_OK(hipSetDevice(dev.id));
        HIP_OK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        const uint64_t n = mcrc_dev::kSmallMax;
        for (Slot &l : slot) {
            if (!l.addr.reserve(n * 8) || !l.len.reserve(n * 4) || !l.cin.reserve(n * 4) || !l.out.reserve(n * 4))
                return CRC32C_ENOMEM;
            HIP_OK(hipEventCreateWithFlags(&l.done, hipEventDisableTiming));
        }
        HIP_OK(hipMalloc(&dnbad, sizeof(unsigned long long)));
        HIP_OK(hipMemset(dnbad, 0, sizeof(unsigned long long)));
        // the dispatcher runs until process exit: an atexit hook (registered
        // after the HIP runtime initialised, so it runs before HIP's static
        // destructors) stops it once the queue has drained and joins it
        worker = std::thread([this] { run(); });
        return CRC32C_OK;
    }

    std::thread worker;
    bool stop = false;  // (under mu)

    void shutdown() {
        {
            std::lock_guard<std::mutex> lk(mu);
            stop = true;
        }
        cv_work.notify_one();
        if (worker.joinable()) worker.join();
    }

    // false once the dispatcher is stopping (process exit): a job queued
    // then might never run, so it is refused instead
    bool submit(crc32c_job *j) {
        {
            std::lock_guard<std::mutex> lk(mu);
            if (stop) return false;
            pending.push_back(j);
        }
        cv_work.notify_one();
        return true;
    }

    // Completion wakes exactly the job's own waiter (a futex on j->done): with
    // many IO threads a shared condition variable woke every waiter per launch,
    // and spinning waiters starved the dispatcher of CPU time.
    // (A spinning waiter can see done == 1, return and free the job before
    // the FUTEX_WAKE below runs.  The wake only hashes the address: on
    // reused memory it at most wakes another job's waiter, which re-checks
    // its word and sleeps again; on unmapped memory it fails with EFAULT.
    // Neither writes memory, so the job is not touched after the store.)
    static void complete(crc32c_job *j, int rc) {
        j->rc = rc;
        j->done.store(1, std::memory_order_release);
        syscall(SYS_futex, reinterpret_cast<int *>(&j->done), FUTEX_WAKE_PRIVATE, 1, nullptr, nullptr, 0);
    }

    static int wait(crc32c_job *j) {
        // a launch completes within tens of microseconds: spin briefly first
        const auto t0 = std::chrono::steady_clock::now();
        while (!j->done.load(std::memory_order_acquire) &&
               std::chrono::steady_clock::now() - t0 < std::chrono::microseconds(10))
            __builtin_ia32_pause();
        while (!j->done.load(std::memory_order_acquire))
            syscall(SYS_futex, reinterpret_cast<int *>(&j->done), FUTEX_WAIT_PRIVATE, 0, nullptr, nullptr, 0);
        return j->rc;
    }

    // The jobs of slot l in one k_small launch over absolute span addresses
    // (enqueued, not waited for).
    int launch(Slot &l) {
        uint64_t k = 0;
        uint64_t *const addr = l.addr.get();
        uint32_t *const len = l.len.get(), *const cin = l.cin.get();
        for (crc32c_job *j : l.jobs) {
            const crc32c_spans &s = j->s;
            for (uint64_t i = 0; i < s.n; ++i, ++k) {
                addr[k] = (uint64_t)(uintptr_t)(j->ptr ? j->views[i] : j->dbase + mcrc::span_off(s, i));
                len[k] = (uint32_t)mcrc::span_len(s, i);
                cin[k] = s.crc_in ? s.crc_in[i] : 0u;
            }
        }
        mcrc_dev::SpanArgs a = common_args(*d, dnbad);
        a.base = nullptr;  // spans at absolute addresses
        a.base_bytes = ~0ull;
        a.offsets = l.addr.dev();
        a.lens = l.len.dev();
        a.crc_in = l.cin.dev();
        a.out = l.out.dev();
        a.n = k;
        int rc = launch_small<0>(*d, a, st);
        if (rc) return rc;
        HIP_OK(hipEventRecord(l.done, st));
        launches.fetch_add(1, std::memory_order_relaxed);
        spans.fetch_add(k, std::memory_order_relaxed);
        jobs.fetch_add(l.jobs.size(), std::memory_order_relaxed);
        return CRC32C_OK;
    }

    // Wait for slot l's launch, hand out the CRCs, wake the waiters.
    void finish(Slot &l, int rc) {
        if (!rc && hipEventSynchronize(l.done) != hipSuccess) rc = CRC32C_EHIP;
        uint64_t k = 0;
        for (crc32c_job *j : l.jobs) {
            if (!rc) memcpy(j->s.out, l.out.get() + k, j->s.n * 4);
            k += j->s.n;
            complete(j, rc);
        }
        l.jobs.clear();
    }

    int run_solo(crc32c_job *j) {
        solo.fetch_add(1, std::memory_order_relaxed);
        if (j->flags & CRC32C_DEVICE) {
            if (j->after) {
                const hipError_t e = hipStreamWaitEvent(st, j->after, 0);
                (void)hipEventDestroy(j->after);
                j->after = nullptr;
                if (e != hipSuccess) return CRC32C_EHIP;
            }
            if (j->ptr) return run_ptr_job(*d, j, st);
            return device_batch(*d, j->s, j->flags & ~(unsigned)CRC32C_ASYNC, st);
        }
        if (j->ptr) return run_ptr_job(*d, j, st);
        return run_host_batch(*d, j->s);
    }

    void run() {
        (void)hipSetDevice(d->id);
        int cur = 0;              // slot of the launch in flight (if it has jobs)
        int rcs[2] = {0, 0};      // launch status of each slot
        for (;;) {
            Slot &busy = slot[cur], &next = slot[cur ^ 1];
            crc32c_job *solo_job = nullptr;
            {
                std::unique_lock<std::mutex> lk(mu);
                if (busy.jobs.empty()) {
                    cv_work.wait(lk, [&] { return !pending.empty() || stop; });
                    if (pending.empty()) return;  // stop, and nothing in flight
                }
                if (!pending.empty() && !pending.front()->coalesce) {
                    solo_job = pending.front();
                    pending.pop_front();
                } else {
                    uint64_t ns = 0;
                    while (!pending.empty() && pending.front()->coalesce &&
                           ns + pending.front()->s.n <= mcrc_dev::kSmallMax) {
                        ns += pending.front()->s.n;
                        next.jobs.push_back(pending.front());
                        pending.pop_front();
                    }
                }
            }
            if (!next.jobs.empty()) rcs[cur ^ 1] = launch(next);  // queued behind the busy slot
            if (!busy.jobs.empty()) finish(busy, rcs[cur]);
            if (solo_job) {  // (the stream is drained first: solo jobs use it too)
                if (!next.jobs.empty()) finish(next, rcs[cur ^ 1]);
                complete(solo_job, run_solo(solo_job));
            }
            cur ^= 1;
        }
    }
};

// Every device's dispatcher stops (after its pending jobs) at process exit.
void stop_queues() {
    std::lock_guard<std::mutex> lk(g_dev_mu);
    for (auto &d : g_devs)
        if (Queue *q = d->queue.load(std::memory_order_acquire)) q->shutdown();
}

int queue_of(Device &d, Queue **out) {
    static std::mutex mu;
    static bool hooked = false;
    std::lock_guard<std::mutex> lk(mu);
    Queue *q = d.queue.load(std::memory_order_acquire);
    if (!q) {
        q = new Queue();
        const int rc = q->init(d);
        if (rc) return rc;  // (a partly initialised queue is leaked, not reused)
        if (!hooked) hooked = std::atexit(stop_queues) == 0;
        d.queue.store(q, std::memory_order_release);
    }
    *out = q;
    return CRC32C_OK;
}

// A new job for the current device's queue; *coalesce says whether it can
// share a launch (host spans, device-visible buffer, short spans).
int make_job(const crc32c_spans &s, unsigned flags, crc32c_job **out) {
    if (s.n && (!s.base || !s.out)) return CRC32C_EINVAL;
    Device *d = nullptr;
    int rc = current_device(&d);
    if (rc) return rc;
    Queue *q = nullptr;
    if ((rc = queue_of(*d, &q))) return rc;
    crc32c_job *j = new crc32c_job();
    j->s = s;
    j->flags = flags & ~(unsigned)CRC32C_ASYNC;
    j->q = q;
    if (flags & CRC32C_DEVICE) {
        // order the job after the submitter's default stream (its work so far)
        if (hipEventCreateWithFlags(&j->after, hipEventDisableTiming) != hipSuccess ||
            hipEventRecord(j->after, nullptr) != hipSuccess) {
            if (j->after) (void)hipEventDestroy(j->after);
            delete j;
            return CRC32C_EHIP;
        }
    } else {
        if (!mcrc::host_spans_ok(s)) {
            delete j;
            return CRC32C_EINVAL;
        }
        bool short_spans = s.n >= 1 && s.n <= mcrc_dev::kSmallMax;
        for (uint64_t i = 0; short_spans && i < s.n; ++i) short_spans = mcrc::span_len(s, i) <= kQueueSpanMax;
        if (short_spans && (j->dbase = device_view_range(s.base, s.base_bytes)) != nullptr) j->coalesce = true;
    }
    *out = j;
    return CRC32C_OK;
}

// crc32c_batch_multi's workers: one persistent thread per gfx950 device,
// bound to its HIP ordinal once (hipSetDevice) when first needed and kept for
// the life of the process (detached; idle ones sleep on their condition
// variable), so a call costs one hand-off per device rather than a thread
// creation and a device bind (round 5 spawned a std::thread per device per
// call).  Each worker runs its parts in the order they were posted; several
// callers may use the pool at once.
struct MultiDone {
    std::mutex mu;
    std::condition_variable cv;
    int left = 0;
    void add() {
        std::lock_guard<std::mutex> lk(mu);
        ++left;
    }
    void finish() {
        std::lock_guard<std::mutex> lk(mu);
        if (--left == 0) cv.notify_all();
    }
    void wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return left == 0; });
    }
};
struct MultiJob {
    crc32c_spans part;
    int *rc;
    MultiDone *done;
};
struct MultiWorker {
    std::mutex mu;
    std::condition_variable cv;
    std::deque<MultiJob> q;
    void post(const MultiJob &j) {
        {
            std::lock_guard<std::mutex> lk(mu);
            q.push_back(j);
        }
        cv.notify_one();
    }
    void run(int ordinal) {
        const bool bound = hipSetDevice(ordinal) == hipSuccess;
        for (;;) {
            MultiJob j;
            {
                std::unique_lock<std::mutex> lk(mu);
                cv.wait(lk, [&] { return !q.empty(); });
                j = q.front();
                q.pop_front();
            }
            *j.rc = bound ? crc32c_batch(&j.part, 0, nullptr) : CRC32C_EHIP;
            j.done->finish();
        }
    }
};
std::mutex g_multi_mu;
MultiWorker *g_multi[kMaxDevices];

MultiWorker *multi_worker(int index) {
    if (index < 0 || index >= kMaxDevices) return nullptr;
    std::lock_guard<std::mutex> lk(g_multi_mu);
    if (!g_multi[index]) {
        const int ordinal = gfx_ordinal(index);
        if (ordinal < 0) return nullptr;
        MultiWorker *w = new MultiWorker();  // (lives for the process)
        std::thread([w, ordinal] { w->run(ordinal); }).detach();
        g_multi[index] = w;
    }
    return g_multi[index];
}

}  // namespace
