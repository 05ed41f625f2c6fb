// hot_queue.h -- the partition queue of hot tiles: BigSeg / BigQueue, the fences and release_lane, job
// emission, record_run, chunk_hist, plan_scatter, cut_pieces and the WIDE job's wide_sort.
// Included by primitives.hip inside namespace hidegs::{anonymous}, after segment_forms.h and queue_trace.h.
#pragma once

// ---- hot tiles: the partition queue --------------------------------------------------------
//
// A segment of more than kSegCap pairs is not sorted by one workgroup (that costs ~10 ns per pair:
// a 100K-pair tile took 1 ms) but split among many.  It becomes a RECORD, partitioned stably by
// one digit -- the top <= 8 bits of (low key half - its MIN) -- in three phases of chunk jobs
// (chunk_size(m) pairs: 4K to 32K by the record's size):
//   REDUCE   MIN / MAX of the chunk's low key halves       -> the digit (last chunk decides)
//   HIST     the chunk's digit counts                      -> pool; the last chunk (of each group
//                                                             of chunks, then of the groups) scans
//                                                             them into every chunk's per-digit
//                                                             destinations
//   SCATTER  the chunk's pairs, ranked stably, to the other buffer (keys <-> alt)
// and the last SCATTER cuts the result into pieces by digit: runs of small digits merged up to
// kSegCap pairs become pieces (the bucket form of segment_sort_kernel, alt -> keys or in place,
// sorted by piece_sort_kernel after the queue; SMALL jobs only if its list is full), a digit of
// kSegCap..kWideCap pairs one WIDE job, a bigger digit a new record one digit lower.  Each level fixes the top <= 8
// varying bits, so the chain ends within 4 levels; pieces left in alt are copied back (COPY jobs).
// Every piece keeps its pairs in input order between equal digits, so the whole is the stable sort.
//
// Jobs live in a queue in scratch, zeroed each call: a producer reserves slots (fetch-add on
// `reserve`), writes them and publishes each by setting its tag; a consumer workgroup claims the next
// index (`head`, relaxed) and waits until that slot is published or every job is finished (`done` == `reserve`:
// nothing in flight, so nothing more can come).  Every wait is bounded (kMaxPolls) and flags
// Q_ERROR when exceeded.  Producers run (they reserved while resident) and publish right after
// writing, so no wait is on a workgroup that is not running.  Ordering across workgroups (and XCD
// L2s) is by agent-scope release / acquire (release_lane / acquire_lane): job payload and pair data
// before the tag, phase data before `pending` and the group countdowns.
constexpr int kChunk = 2 * kBigStep;  // pairs per chunk job of a small record
// A bigger record's chunk jobs take 2, 4 or 8 kChunk pieces each: a job's hand-off (claim, acquire,
// release) costs ~10 us whatever its size, so the 2100 chunk jobs per phase of an 8.6M-pair tile
// spent most of their time in hand-offs (tools/gpu_queue_ab.sh: DESIGN.md "A known limit").
constexpr uint32_t kChunkX2 = 32768, kChunkX4 = 131072, kChunkX8 = 1048576;  // records over these many pairs
static_assert((kChunk & (kChunk - 1)) == 0, "chunk sizes are kChunk << 0..3");
__device__ __forceinline__ uint32_t chunk_size(uint32_t m)
{
    return (uint32_t)kChunk << (m > kChunkX8 ? 3 : m > kChunkX4 ? 2 : m > kChunkX2 ? 1 : 0);
}
constexpr int kQueueBlocks = 256;      // queue workers
constexpr uint32_t kBackoffMax = 16;   // a waiting worker's longest sleep between polls, in s_sleep(8) units
constexpr int kWideCap = 12288;        // segments up to this many pairs: one WIDE job (LDS sort by one worker)
constexpr int kPieceWaves = 5;  // waves per SIMD piece_sort_kernel's register budget is set for (6: 10 VGPRs spilled)
// The -D knobs of the test variants (hidegs_amd/build.py VARIANTS):
#ifndef HIDEGS_QUEUE_MIN
#define HIDEGS_QUEUE_MIN 2048  // segments up to this many pairs: the one-workgroup global form (2048 = kSegCap:
                              // every tile over kSegCap goes to the queue; tools/skew_time.py A/B in DESIGN.md)
#endif
constexpr int kQueueMin = HIDEGS_QUEUE_MIN;
#ifndef HIDEGS_WIDE_SCOUTS
#define HIDEGS_WIDE_SCOUTS 0  // 1: scouts hand hot tiles of <= kWideCap pairs to the queue as WIDE jobs (slower: DESIGN.md)
#endif
#ifndef HIDEGS_MAX_POLLS
#define HIDEGS_MAX_POLLS (1u << 22)  // a waiting worker gives up after this many polls (~13 s at the longest backoff)
#endif
constexpr uint32_t kMaxPolls = HIDEGS_MAX_POLLS;
enum : uint32_t { J_EXIT = 0, J_SMALL, J_COPY, J_REDUCE, J_HIST, J_SCATTER, J_GLOBAL, J_WIDE };
enum : int { Q_HEAD, Q_RESERVE, Q_DONE, Q_NREC, Q_POOL, Q_ERROR, Q_NPIECE, Q_COUNTERS = 8 };
constexpr int kCtlStride = 32;  // one 128-byte line per counter: polls of one do not queue behind another's atomics
constexpr int Q_WORDS = Q_COUNTERS * kCtlStride;
static_assert(Q_WORDS <= kBlock, "identify_ranges_kernel zeroes the counters with one workgroup");

struct BigSeg {
    uint32_t begin, m, src, chunks;  // pairs [begin, begin + m) of keys (src 0) or alt (src 1)
    uint32_t lo_bits, hi_bits;       // REDUCE: MIN / MAX of the low key halves
    uint32_t shift, bits;            // the digit: bits [shift, shift + bits) of (low key half - lo)
    uint32_t lo;                     // the digit's base: the record's smallest low key half
    uint32_t pool;                   // (chunks + 2) x 256 u32: per-chunk counts -> destinations,
                                     // then the digit starts and the digit totals
    uint32_t pending;                // jobs of the current phase not yet finished
    uint32_t csize;                  // pairs per chunk job (chunk_size(m))
};

struct BigQueue {
    uint32_t* ctl;  // Q_WORDS counters, zeroed before segment_sort_kernel
    BigSeg* rec;
    uint4* job;     // (type | src << 8, a, b, tag): tag 1 once published (zeroed each call)
    uint32_t* pool;
    uint32_t rec_cap, job_cap, pool_cap;
    uint64_t* alt_k;  // the sort's alternate buffers (the global form of a mildly hot tile)
    uint32_t* alt_v;
    uint2* piece;     // deferred pieces (begin, m | src << 31) for piece_sort_kernel
    uint32_t piece_cap;
};

__device__ __forceinline__ uint32_t q_load(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT); }
// polling reads: coherent but without the acquire's cache invalidation (taken once, after the wait)
__device__ __forceinline__ uint32_t q_peek(uint32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void fence_acquire() { __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent"); }
__device__ __forceinline__ void fence_release() { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent"); }
// Cache maintenance is per CU (L1) and per XCD (L2), not per wave, and it is costly (an L2
// writeback or invalidate per fence; with fences in every wave of every job the chain of a 500K-pair
// tile ran 1.2 ms): each wave only waits for its own stores to be acknowledged, then after a barrier
// ONE thread's agent-scope release (L2 writeback) or acquire (invalidate) acts for the workgroup.
__device__ __forceinline__ void wave_stores_done() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// ONE lane's release for its workgroup (after every storing wave's wave_stores_done and a barrier),
// before the flag, tag or count that publishes the stores.  The explicit wait after the L2 writeback
// is not redundant: ROCm 7.2 drops the compiler's own wait after `buffer_wbl2` when it thinks the
// wave has nothing outstanding, and the count then overtakes the write-back (a group countdown built
// that way let a reader on another XCD scan stale count rows: an illegal address under load).
__device__ __forceinline__ void release_lane()
{
    fence_release();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// ONE lane's acquire for its workgroup, after its relaxed poll matched or its countdown came last;
// the wait completes the L1 invalidate before the barrier that lets the other waves load.
__device__ __forceinline__ void acquire_lane()
{
    fence_acquire();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}
// Sticky per-device copy of every queue error (bit 1: job slots exhausted, bit 4: a worker gave up
// waiting), read and cleared by hidegs_queue_error(); the debug mode (hidegs_set_debug) checks it after
// every sort.  A set bit means the sort's output is not trustworthy.
__device__ uint32_t g_queue_error;
__device__ __forceinline__ void q_flag(const BigQueue& q, uint32_t bit)
{
    __hip_atomic_fetch_or(&q.ctl[kCtlStride * Q_ERROR], bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_or(&g_queue_error, bit, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Jobs a workgroup is about to enqueue, as runs: `count` jobs of one kind.
constexpr int kMaxRuns = kRadix + 1;
struct EmitShared {
    uint4 run[kMaxRuns];  // (type | src << 8, a, b, count)
    uint32_t off[kMaxRuns + 1];
    uint32_t nruns, base, pbase;
};

__device__ __forceinline__ void runs_begin(EmitShared& e)
{
    e.nruns = 0;
    e.off[0] = 0;
}

__device__ __forceinline__ void add_run(EmitShared& e, uint32_t type, uint32_t src, uint32_t a, uint32_t b,
                                        uint32_t count)
{
    if (count == 0) return;
    e.run[e.nruns] = make_uint4(type | (src << 8), a, b, count);
    e.off[e.nruns + 1] = e.off[e.nruns] + count;
    e.nruns++;
}

// Job j of a run: chunk j of a record, the j-th kChunk piece of a COPY range, or the one job.
__device__ __forceinline__ uint4 run_job(const uint4 r, const uint32_t j)
{
    const uint32_t type = r.x & 0xffu;
    if (type == J_COPY) {
        const uint32_t s = j * kChunk;
        return make_uint4(r.x, r.y + s, r.z - s < (uint32_t)kChunk ? r.z - s : (uint32_t)kChunk, 0u);
    }
    if (type == J_REDUCE || type == J_HIST || type == J_SCATTER) return make_uint4(r.x, r.y, j, 0u);
    return make_uint4(r.x, r.y, r.z, 0u);
}

// A record's digit over its low keys' range [lo, hi] (lo < hi): the top <= 8 bits of x - lo.  Float
// depth bits that cross exponent boundaries vary in every exponent bit; a digit of the top varying
// bits would then split by exponent only (a few crowded digits), one of the range splits the mass.
__device__ __forceinline__ void range_digit(uint32_t lo, uint32_t hi, int& shift, int& bits)
{
    const int nbits = 32 - __builtin_clz(hi - lo);
    bits = nbits < kRadixBits ? nbits : kRadixBits;
    shift = nbits - bits;
}
__device__ __forceinline__ void set_digit(BigSeg& s, uint32_t lo, uint32_t hi)
{
    int shift, bits;
    range_digit(lo, hi, shift, bits);
    s.lo = lo;
    s.shift = (uint32_t)shift;
    s.bits = (uint32_t)bits;
}
// digit of a pair of a record: bits [shift, shift + bits) of (low key half - lo)
__device__ __forceinline__ uint32_t rec_digit(uint32_t key_lo, uint32_t lo, int shift, uint32_t mask)
{
    return ((key_lo - lo) >> shift) & mask;
}
// The low half of keys[i], as a 4-byte load: what the phases that look at digits only (REDUCE, HIST) read.
// segment_sort_kernel<true>'s scouts run them while the tile's own workgroup rewrites the high halves
// (expand_records); the low halves keep their values.
__device__ __forceinline__ uint32_t key_low(const uint64_t* keys, uint32_t i)
{
    return reinterpret_cast<const uint32_t*>(keys)[2 * (size_t)i];
}

// Chunk groups of a big record.  The SCATTER phase needs, per chunk and digit, the digit's count in
// the chunks before it: one workgroup walking the digit columns of all chunks took 246 us for a
// 8.5M-pair record (2100 dependent rows).  A record of more than kGroupChunks chunks therefore
// counts its HIST phase down per group: the last chunk of a group turns the group's counts into
// prefixes within the group and its sum row, the last group plans the groups' bases (<= 256 rows).
constexpr uint32_t kGroupChunks = 32;
__device__ __forceinline__ uint32_t group_chunks(uint32_t chunks)
{
    const uint32_t g = (chunks + kRadix - 1) / kRadix;  // at most 256 groups
    return g > kGroupChunks ? g : kGroupChunks;
}
__device__ __forceinline__ uint32_t num_groups(uint32_t chunks)  // 0: an ungrouped record
{
    return chunks > kGroupChunks ? (chunks + group_chunks(chunks) - 1) / group_chunks(chunks) : 0u;
}
// Pool rows of a record: [0, chunks) per-chunk counts -> destinations (grouped: prefixes within the
// group), chunks + 0..3 the digit starts, totals, MIN and MAX, then (grouped) one row per group (its
// sums -> its bases) and one row of group countdowns.
__device__ __forceinline__ uint32_t pool_rows(uint32_t chunks)
{
    // num_groups(chunks) <= chunks / kGroupChunks + 1 (a bound without branches: the exact count
    // here cost segment_sort_kernel, where the scouts open records, 4 spilled VGPRs)
    return chunks + 4 + chunks / kGroupChunks + 2;
}
// One thread: a record's HIST countdown (chunks, or its groups with each group's own countdown);
// the stores are published by the emit_jobs that queues the HIST jobs.
__device__ __forceinline__ uint32_t hist_countdown(const BigQueue& q, const BigSeg& s)
{
    const uint32_t ng = num_groups(s.chunks);
    if (ng == 0) return s.chunks;
    const uint32_t G = group_chunks(s.chunks);
    uint32_t* down = q.pool + s.pool + (s.chunks + 4 + ng) * kRadix;
    for (uint32_t g = 0; g < ng; g++) down[g] = s.chunks - g * G < G ? s.chunks - g * G : G;
    return ng;
}

// A new record over [begin, begin + m) of buffer src, as the run of jobs that starts it: REDUCE
// chunk jobs, or -- when the low keys' range [lo, hi] is known already (from the parent's SCATTER or
// the opener; `known` false: unknown) -- HIST chunk jobs right away, or a COPY / nothing for a piece
// of equal low keys.  With the record table or the pool full: one GLOBAL job (the one-workgroup sort).
// The pool holds pool_rows(chunks) x 256 u32: per-chunk counts -> destinations, then the digit
// starts, totals, and MIN / MAX of each digit's low key halves (the next level's range), and the
// rows of the chunk groups.
template <bool Grouped = true>  // false: the caller knows m <= kGroupChunks chunks (no countdowns)
__device__ __forceinline__ uint4 record_run(const BigQueue& q, uint32_t begin, uint32_t m, uint32_t src,
                                            bool known, uint32_t lo, uint32_t hi)
{
    if (known && lo == hi)  // already in order
        return make_uint4(J_COPY | (src << 8), begin, m, src ? (m + kChunk - 1) / kChunk : 0u);
    const uint32_t csize = Grouped ? chunk_size(m) : (uint32_t)kChunk;
    const uint32_t chunks = (m + csize - 1) >> (31 - __builtin_clz(csize));
    const uint32_t need = (Grouped ? pool_rows(chunks) : chunks + 4) * kRadix;
    const uint32_t r = __hip_atomic_fetch_add(&q.ctl[kCtlStride * Q_NREC], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    uint32_t p = ~0u;
    if (r < q.rec_cap) {
        p = __hip_atomic_fetch_add(&q.ctl[kCtlStride * Q_POOL], need, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint64_t)p + need > q.pool_cap) p = ~0u;
    }
    if (p == ~0u) return make_uint4(J_GLOBAL | (src << 8), begin, m, 1u);
    BigSeg& s = q.rec[r];
    s.begin = begin;
    s.m = m;
    s.src = src;
    s.chunks = chunks;
    s.lo_bits = 0xffffffffu;
    s.hi_bits = 0u;  // shift, bits and lo: set_digit, before the first HIST job reads them
    s.pool = p;
    s.pending = chunks;
    s.csize = csize;
    if (!known) return make_uint4(J_REDUCE, r, 0u, chunks);
    set_digit(s, lo, hi);
    if (Grouped) s.pending = hist_countdown(q, s);
    return make_uint4(J_HIST, r, 0u, chunks);
}

__device__ __forceinline__ void add_run(EmitShared& e, const uint4 r) { add_run(e, r.x & 0xffu, r.x >> 8, r.y, r.z, r.w); }

// All threads: enqueue the runs thread 0 put in e (its writes precede the first barrier).
__device__ __forceinline__ void emit_jobs(const BigQueue& q, EmitShared& e)
{
    const int t = threadIdx.x;
    __syncthreads();
    const uint32_t nr = e.nruns, total = e.off[nr];
    if (total == 0) return;  // block-uniform
    if (t == 0) {
        // fetch-add, not a CAS loop: 80 records of one level reserving at once retried their CAS
        // for 160 us
        uint32_t base = __hip_atomic_fetch_add(&q.ctl[kCtlStride * Q_RESERVE], total, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
        if ((uint64_t)base + total > q.job_cap) {  // beyond the capacity bound of sort_scratch: cannot
            q_flag(q, 1u);                          // happen; count the lost jobs done so the queue ends
            __hip_atomic_fetch_add(&q.ctl[kCtlStride * Q_DONE], total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            base = ~0u;
        }
        e.base = base;
    }
    __syncthreads();
    const uint32_t base = e.base;
    if (base == ~0u) return;
    for (uint32_t j = t; j < total; j += kBlock) {
        // the run holding job j: off[r] <= j < off[r + 1] (a binary search -- a linear walk over a
        // split record's 256 runs cost its last SCATTER job ~60 us of dependent LDS reads)
        uint32_t r = 0, hi = nr;
        while (hi - r > 1u) {
            const uint32_t mid = (r + hi) >> 1;
            if (e.off[mid] <= j) r = mid; else hi = mid;
        }
        q.job[base + j] = run_job(e.run[r], j - e.off[r]);  // tag (.w) 0: not yet published
    }
    wave_stores_done();  // the jobs (and record / pool / pair stores) before the publish below
    __syncthreads();
    if (t == 0) release_lane();  // one L2 writeback for the workgroup (see wave_stores_done)
    __syncthreads();
    // publish: each slot's tag becomes 1 (slots publish independently -- a global publication
    // order would chain every producer behind the one that reserved before it: 80 records of one
    // level published one after another took 300 us)
    for (uint32_t j = t; j < total; j += kBlock)
        __hip_atomic_store(&q.job[base + j].w, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Thread t's result: the number of the cnt keys at sk[base..] whose digit is t (U x kChunk keys
// loaded at a time: the queue's workers, one wave per SIMD, take U = 4; open_local, inside
// segment_sort_kernel's 72-VGPR budget, 1).
constexpr int kQueueIlp = 4;
template <int U = 1>
__device__ __forceinline__ uint32_t chunk_hist(const uint64_t* sk, const uint32_t base, const uint32_t cnt,
                                               const uint32_t lo, const int shift, const uint32_t mask, BigShared& sh)
{
    const int t = threadIdx.x;
    sh.hist[t] = 0u;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < cnt; i0 += U * kChunk) {
        uint32_t dg[U * kChunk / kBlock];
#pragma unroll
        for (int u = 0; u < U * kChunk / kBlock; u++) {
            const uint32_t i = i0 + t + u * kBlock;
            dg[u] = i < cnt ? rec_digit(key_low(sk, base + i), lo, shift, mask) : ~0u;
        }
#pragma unroll
        for (int u = 0; u < U * kChunk / kBlock; u++)
            if (dg[u] != ~0u) atomicAdd(&sh.hist[dg[u]], 1u);
    }
    __syncthreads();
    return sh.hist[t];
}

// Rows [r0, r0 + n) of this thread's digit column: each count becomes base + the counts before it
// (an exclusive scan down the column); returns the column's sum.
__device__ __forceinline__ uint32_t scan_column(uint32_t* col, const uint32_t r0, const uint32_t n, uint32_t base)
{
    constexpr uint32_t U = 8;  // independent loads in flight: the column is in other XCDs' writes
    for (uint32_t j0 = 0; j0 < n; j0 += U) {
        uint32_t x[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) x[u] = j0 + u < n ? col[(r0 + j0 + u) * kRadix] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < U; u++) {
            if (j0 + u < n) col[(r0 + j0 + u) * kRadix] = base;
            base += x[u];
        }
    }
    return base;
}

// After every chunk's counts are in the record's pool (col = this thread's digit column) -- for a
// grouped record, every group's sums (the chunks' rows hold prefixes within their group): every
// chunk's (group's) destination of each digit (begin + digit start + the digit's count in the chunks
// (groups) before it), the digit starts and totals, and the MIN / MAX rows the SCATTER jobs gather into.
template <bool Grouped = true>  // false: the caller knows the record is ungrouped
__device__ __forceinline__ void plan_scatter(uint32_t* col, const uint32_t chunks, const uint32_t begin, BigShared& sh)
{
    constexpr uint32_t U = 8;
    const uint32_t ng = Grouped ? num_groups(chunks) : 0u;
    const uint32_t r0 = ng ? chunks + 4 : 0u, n = ng ? ng : chunks;
    uint32_t tot = 0u;
    for (uint32_t j0 = 0; j0 < n; j0 += U) {
        uint32_t x[U];
#pragma unroll
        for (uint32_t u = 0; u < U; u++) x[u] = j0 + u < n ? col[(r0 + j0 + u) * kRadix] : 0u;
#pragma unroll
        for (uint32_t u = 0; u < U; u++) tot += x[u];
    }
    uint32_t dummy;
    const uint32_t start = block_exclusive_scan(tot, sh.wave, &dummy);
    scan_column(col, r0, n, begin + start);
    col[chunks * kRadix] = start;
    col[(chunks + 1) * kRadix] = tot;
    col[(chunks + 2) * kRadix] = 0xffffffffu;
    col[(chunks + 3) * kRadix] = 0u;
}

// The last chunk of a record's SCATTER phase (all of its pairs are in buffer dst, and col -- this
// thread's digit column of the record's pool -- holds the digit starts, totals and MIN / MAX rows):
// cut the record into the pieces the queue sorts next, as runs in e (thread 0 publishes them with
// emit_jobs).  Every thread of the workgroup calls it.
__device__ __forceinline__ void cut_pieces(const BigQueue& q, EmitShared& e, BigShared& sh, const uint32_t* col,
                                           const uint32_t chunks, const uint32_t begin, const uint32_t m,
                                           const int shift, const uint32_t dst)
{
    const int t = threadIdx.x;
    // cut the record into pieces, one thread per digit:
    //  * a digit of more than kSegCap pairs: a record of the next level (its varying
    //    bits are known: HIST jobs directly);
    //  * a digit of more than kSegRun pairs: a SMALL piece of its own;
    //  * other non-empty digits: SMALL pieces of consecutive digits whose starts share
    //    a kSegRun-aligned window (so a piece holds < 2 * kSegRun = kSegCap pairs).
    const uint32_t n_d = col[(chunks + 1) * kRadix];  // 0 above the digit mask
    const uint32_t s_d = col[chunks * kRadix];        // relative start
    const uint32_t lo_d = col[(chunks + 2) * kRadix], hi_d = col[(chunks + 3) * kRadix];  // the digit's range
    if (shift == 0) {  // every varying bit is placed: the record is sorted
        if (t == 0) {
            runs_begin(e);
            if (dst) add_run(e, J_COPY, 1u, begin, m, (m + kChunk - 1) / kChunk);  // kChunk pieces
        }
    } else {
        const bool nonempty = n_d != 0u, solo = n_d > (uint32_t)kSegRun;
        uint32_t* pv = sh.hist;  // previous non-empty digit + 1: inclusive max-scan
        uint32_t* nx = sh.run;   // start of the next piece: suffix min-scan
        pv[t] = nonempty ? (uint32_t)t + 1u : 0u;
        sh.cnt[0][t] = solo;
        sh.cnt[1][t] = s_d;
        __syncthreads();
        for (int o = 1; o < kRadix; o <<= 1) {
            const uint32_t x = t >= o ? pv[t - o] : 0u;
            __syncthreads();
            pv[t] = x > pv[t] ? x : pv[t];
            __syncthreads();
        }
        const uint32_t prev = t ? pv[t - 1] : 0u;
        const bool boundary = nonempty && (prev == 0u || solo || sh.cnt[0][prev - 1] != 0u ||
                                           (s_d / kSegRun) != (sh.cnt[1][prev - 1] / kSegRun));
        nx[t] = boundary ? s_d : m;
        __syncthreads();
        for (int o = 1; o < kRadix; o <<= 1) {
            const uint32_t x = t + o < kRadix ? nx[t + o] : m;
            __syncthreads();
            nx[t] = x < nx[t] ? x : nx[t];
            __syncthreads();
        }
        const uint32_t next = t + 1 < kRadix ? nx[t + 1] : m;
        uint4 run = make_uint4(0u, 0u, 0u, 0u);
        bool piece = false;
        if (boundary) {
            if (n_d > (uint32_t)kSegCap)
                run = n_d <= (uint32_t)kWideCap ? make_uint4(J_WIDE | (dst << 8), begin + s_d, n_d, 1u)
                                                : record_run(q, begin + s_d, n_d, dst, true, lo_d, hi_d);
            else if (next - s_d > 1u || dst)
                piece = true;
        }
        // pieces go to piece_sort_kernel's list (a SMALL job only if it is full)
        uint32_t npc;
        const uint32_t pi = block_exclusive_scan(piece ? 1u : 0u, sh.wave, &npc);
        if (npc) {  // workgroup-uniform
            if (t == 0)
                e.pbase = __hip_atomic_fetch_add(&q.ctl[kCtlStride * Q_NPIECE], npc, __ATOMIC_RELAXED,
                                                 __HIP_MEMORY_SCOPE_AGENT);
            __syncthreads();
            if (piece) {
                const uint32_t k = e.pbase + pi;
                if (k < q.piece_cap)
                    q.piece[k] = make_uint2(begin + s_d, (next - s_d) | (dst << 31));
                else
                    run = make_uint4(J_SMALL | (dst << 8), begin + s_d, next - s_d, 1u);
            }
        }
        uint32_t nruns, total;
        const uint32_t ri = block_exclusive_scan(run.w ? 1u : 0u, sh.wave, &nruns);
        const uint32_t ro = block_exclusive_scan(run.w, sh.wave, &total);
        if (run.w) {
            e.run[ri] = run;
            e.off[ri] = ro;
        }
        if (t == 0) {
            e.nruns = nruns;
            e.off[nruns] = total;
        }
    }
}

// A WIDE job: one segment of kSegCap < m <= kWideCap pairs sorted whole by ONE queue worker in LDS
// (big_segment_kernel runs at one workgroup per CU, so it can hold 152 KB): the hot tiles of a skewed
// view and the level-1 digits of a very hot one, each in one job instead of a record's chain of
// REDUCE / HIST / SCATTER hand-offs and pieces (tools/skew_time.py: DESIGN.md "Skewed views").
constexpr int kWideRounds = 4;  // 64-item rounds a wave ranks at once
constexpr int kWideBatch = 8;  // global loads in flight per thread in the load and gather loops
constexpr int kWideIndexBits = 14;
constexpr int kWideIlp = 4;  // items per thread in flight in the bucket form's LDS phases
constexpr int kWideMaxBucket = 128;  // a fuller bucket sends the WIDE segment to the LSD passes
struct WideShared {
    uint32_t k[2][kWideCap];  // low key halves
    uint16_t i[2][kWideCap];  // index in the segment
    uint32_t cnt[kWavesPerBlock][kRadix];
    uint32_t wave[kWavesPerBlock];
    uint32_t red[2][kWavesPerBlock];
};
static_assert(kWideCap <= (1 << kWideIndexBits) && kWideCap % kBlock == 0, "WIDE segment indices are u16 / 14 bits");
static_assert(2 * kBuckets * sizeof(uint32_t) <= sizeof(uint16_t) * kWideCap, "bucket counters fit in i[0]");

// Pairs [begin, begin + m) of (src ? alt : keys) sorted stably by their low 32 key bits into
// keys / vals (m <= kWideCap).  The low halves and indices are sorted in LDS by stable 8-bit LSD
// passes over the bits that vary (per pass: per-wave digit counts, their scan, then each wave ranks
// its contiguous share in input order with wave_rank); the pairs are then gathered by index from alt
// (src 0: copied there first, so keys can be written in place).
__device__ __forceinline__ void wide_sort(uint64_t* __restrict__ keys, uint32_t* __restrict__ vals,
                                          uint64_t* __restrict__ alt_k, uint32_t* __restrict__ alt_v,
                                          const uint32_t begin, const uint32_t m, const uint32_t src, WideShared& w)
{
    const int t = threadIdx.x, lane = lane_id(), wave = t / kWave;
    const uint64_t* sk = src ? alt_k : keys;
#ifdef HIDEGS_QUEUE_TRACE
    __shared__ unsigned int s_wslot;
    if (t == 0) {
        s_wslot = atomicAdd(&g_wtrace_n, 1u);
        if (s_wslot < kWTraceCap) g_wtrace[s_wslot][0] = m;
    }
    __syncthreads();
    const unsigned int wslot = s_wslot;
#endif
    WSTAMP(0);
    uint32_t a = 0xffffffffu, o = 0u, mn = 0xffffffffu, mx = 0u;
    for (uint32_t i0 = 0; i0 < m; i0 += kBlock * kWideBatch) {  // kWideBatch loads in flight per thread
        uint64_t kk[kWideBatch];
        uint32_t vv[kWideBatch];
#pragma unroll
        for (int u = 0; u < kWideBatch; u++) {
            const uint32_t i = i0 + u * kBlock + t;
            if (i < m) {
                kk[u] = sk[begin + i];
                if (!src) vv[u] = vals[begin + i];
            }
        }
#pragma unroll
        for (int u = 0; u < kWideBatch; u++) {
            const uint32_t i = i0 + u * kBlock + t;
            if (i < m) {
                const uint32_t lo = (uint32_t)kk[u];
                w.k[0][i] = lo;
                w.i[0][i] = (uint16_t)i;
                a &= lo;
                o |= lo;
                mn = min(mn, lo);
                mx = max(mx, lo);
                if (!src) {
                    alt_k[begin + i] = kk[u];
                    alt_v[begin + i] = vv[u];
                }
            }
        }
    }
    const SegStats st = segment_stats(a, o, mn, mx, w.red[0], w.red[1]);
    const uint32_t diff = st.diff;  // block-uniform
    WSTAMP(1);
    int cur = 0;
    // Bucket form (as segment_sort's): (x - lo) >> shift over the segment's key range picks a bucket,
    // and an item's place in its bucket is its exact rank by (the bits below || index), so equal keys
    // keep their input order.  Its start / fill counters borrow the storage of i[0].
    const int bshift = st.shift;
    const uint32_t base_lo = st.lo;
    bool lsd = diff != 0u;
    if (diff && bshift + kWideIndexBits <= 32) {  // block-uniform
        const uint32_t lowmask = (uint32_t)((1ull << bshift) - 1ull);
        uint32_t* start = reinterpret_cast<uint32_t*>(&w.i[0][0]);
        uint32_t* fill = start + kBuckets;
        for (int b = t; b < kBuckets; b += kBlock) fill[b] = 0u;
        __syncthreads();
        for (uint32_t i0 = 0; i0 < m; i0 += kWideIlp * kBlock) {  // kWideIlp independent items per thread
            uint32_t x[kWideIlp];
#pragma unroll
            for (int u = 0; u < kWideIlp; u++) {
                const uint32_t i = i0 + u * kBlock + t;
                x[u] = i < m ? w.k[0][i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < kWideIlp; u++)
                if (i0 + u * kBlock + t < m) atomicAdd(&fill[(x[u] - base_lo) >> bshift], 1u);
        }
        __syncthreads();
        WSTAMP(2);
        uint32_t c[kBuckets / kBlock], sum = 0, mx = 0;
#pragma unroll
        for (int j = 0; j < kBuckets / kBlock; j++) {
            c[j] = fill[t * (kBuckets / kBlock) + j];
            sum += c[j];
            mx = c[j] > mx ? c[j] : mx;
        }
        uint32_t dummy;
        uint32_t pre = block_exclusive_scan(sum, w.wave, &dummy);  // its barriers order the reads above
#pragma unroll
        for (int sft = 32; sft >= 1; sft >>= 1) {
            const uint32_t y = __shfl_xor(mx, sft, kWave);
            mx = y > mx ? y : mx;
        }
        if (lane == 0) w.red[0][wave] = mx;
#pragma unroll
        for (int j = 0; j < kBuckets / kBlock; j++) {
            start[t * (kBuckets / kBlock) + j] = pre;
            fill[t * (kBuckets / kBlock) + j] = pre;
            pre += c[j];
        }
        __syncthreads();
        uint32_t fullest = 0;
#pragma unroll
        for (int ww = 0; ww < kWavesPerBlock; ww++) fullest = w.red[0][ww] > fullest ? w.red[0][ww] : fullest;
        WSTAMP(3);
        if (fullest <= (uint32_t)kWideMaxBucket) {  // block-uniform
            uint32_t* comb = w.k[1];
            for (uint32_t i0 = 0; i0 < m; i0 += kWideIlp * kBlock) {
                uint32_t x[kWideIlp], slot[kWideIlp];
#pragma unroll
                for (int u = 0; u < kWideIlp; u++) {
                    const uint32_t i = i0 + u * kBlock + t;
                    x[u] = i < m ? w.k[0][i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < kWideIlp; u++)
                    if (i0 + u * kBlock + t < m) slot[u] = atomicAdd(&fill[(x[u] - base_lo) >> bshift], 1u);
#pragma unroll
                for (int u = 0; u < kWideIlp; u++) {
                    const uint32_t i = i0 + u * kBlock + t;
                    if (i < m) comb[slot[u]] = (((x[u] - base_lo) & lowmask) << kWideIndexBits) | i;
                }
            }
            __syncthreads();
            WSTAMP(4);
            for (uint32_t i0 = 0; i0 < m; i0 += kWideIlp * kBlock) {
                uint32_t me[kWideIlp], s0[kWideIlp], e0[kWideIlp], rank[kWideIlp];
                uint32_t len = 0;
#pragma unroll
                for (int u = 0; u < kWideIlp; u++) {
                    const uint32_t i = i0 + u * kBlock + t;
                    const uint32_t x = (i < m ? w.k[0][i] : base_lo) - base_lo;
                    const uint32_t bk = x >> bshift;
                    me[u] = ((x & lowmask) << kWideIndexBits) | i;
                    s0[u] = start[bk];
                    e0[u] = i < m ? fill[bk] : s0[u];
                    rank[u] = 0u;
                    len = e0[u] - s0[u] > len ? e0[u] - s0[u] : len;
                }
                for (uint32_t j = 0; j < len; j++) {  // the kWideIlp bucket walks interleaved
#pragma unroll
                    for (int u = 0; u < kWideIlp; u++)
                        if (s0[u] + j < e0[u]) rank[u] += comb[s0[u] + j] < me[u] ? 1u : 0u;
                }
#pragma unroll
                for (int u = 0; u < kWideIlp; u++)
                    if (i0 + u * kBlock + t < m) w.i[1][s0[u] + rank[u]] = (uint16_t)(i0 + u * kBlock + t);
            }
            __syncthreads();
            WSTAMP(5);
            cur = 1;
            lsd = false;
        } else {  // crowded buckets: the LSD passes below, whose i[0] the counters overwrote
            for (uint32_t i = t; i < m; i += kBlock) w.i[0][i] = (uint16_t)i;
            __syncthreads();
        }
    }
    const uint32_t C = (m + kBlock - 1) / kBlock * kWave;  // each wave's contiguous share (64-item rounds)
    const uint32_t w0 = wave * C, w1 = w0 + C < m ? w0 + C : m;
    for (int shift = 0; shift < 32 && lsd; shift += kRadixBits) {
        const uint32_t vary = (diff >> shift) & (kRadix - 1);
        if (vary == 0) continue;  // digit constant over the segment (block-uniform)
        for (int i = t; i < kWavesPerBlock * kRadix; i += kBlock) (&w.cnt[0][0])[i] = 0u;
        __syncthreads();
        for (uint32_t i0 = w0; i0 < w1; i0 += 4 * kWave) {
            uint32_t x[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t i = i0 + u * kWave + lane;
                x[u] = i < w1 ? w.k[cur][i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < 4; u++)
                if (i0 + u * kWave + lane < w1) atomicAdd(&w.cnt[wave][(x[u] >> shift) & (kRadix - 1)], 1u);
        }
        __syncthreads();
        const uint32_t tot = digit_wave_prefix(w.cnt);  // cnt[ww][d]: digit d in waves before ww
        uint32_t dummy;
        const uint32_t start = block_exclusive_scan(tot, w.wave, &dummy);  // its barriers order the above
#pragma unroll
        for (int ww = 0; ww < kWavesPerBlock; ww++) w.cnt[ww][t] += start;  // thread t owns digit t
        __syncthreads();
        for (uint32_t r0 = w0; r0 < w1; r0 += kWideRounds * kWave) {  // wave-uniform
            uint32_t kk[kWideRounds], id[kWideRounds], rank[kWideRounds];
            bool ok[kWideRounds];
#pragma unroll
            for (int q = 0; q < kWideRounds; q++) {
                const uint32_t i = r0 + q * kWave + lane;
                ok[q] = i < w1;
                kk[q] = ok[q] ? w.k[cur][i] : 0u;
                id[q] = ok[q] ? w.i[cur][i] : 0u;
            }
            // cnt starts at each digit's first position for this wave: rank = the item's position
            wave_rank<uint32_t, kWideRounds>(kk, ok, shift, kRadix - 1, w.cnt[wave], rank, vary);
#pragma unroll
            for (int q = 0; q < kWideRounds; q++) {
                if (ok[q]) {
                    w.k[cur ^ 1][rank[q]] = kk[q];
                    w.i[cur ^ 1][rank[q]] = (uint16_t)id[q];
                }
            }
        }
        __syncthreads();
        cur ^= 1;
    }
    WSTAMP(6);
    if (!diff && !src) return;  // equal low keys, in place: the input order is the stable order
    for (uint32_t j0 = 0; j0 < m; j0 += kBlock * kWideBatch) {
        uint32_t ii[kWideBatch];
        uint64_t kk[kWideBatch];
        uint32_t vv[kWideBatch];
#pragma unroll
        for (int u = 0; u < kWideBatch; u++) {
            const uint32_t j = j0 + u * kBlock + t;
            ii[u] = j < m ? w.i[cur][j] : 0u;
        }
#pragma unroll
        for (int u = 0; u < kWideBatch; u++) {
            if (j0 + u * kBlock + t < m) {
                kk[u] = alt_k[begin + ii[u]];
                vv[u] = alt_v[begin + ii[u]];
            }
        }
#pragma unroll
        for (int u = 0; u < kWideBatch; u++) {
            const uint32_t j = j0 + u * kBlock + t;
            if (j < m) {
                keys[begin + j] = kk[u];
                vals[begin + j] = vv[u];
            }
        }
    }
#ifdef HIDEGS_QUEUE_TRACE
    wave_stores_done();
    __syncthreads();
#endif
    WSTAMP(7);
}
