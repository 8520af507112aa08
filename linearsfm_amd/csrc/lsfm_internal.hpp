// Host-side internals of liblsfm_hip: context, device arenas, the batched map container and stage entry points.
//
// Design: all maps of one tree level live in ONE flat structure-of-arrays container on the device
// ("DevBatch"); pose / feature indices inside U and W are GLOBAL indices into that container, so a kernel
// processes every map of the level in a single launch and a pairwise join is mostly a re-indexing of features.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <condition_variable>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <thread>
#include <string>
#include <vector>

#include "../../include/lsfm.h"
#include "lsfm_map.hpp"

namespace lsfm {

struct Error { int code; std::string msg; };
struct DevBatch;
struct IndexHold;    // device memory a plan owns (lsfm_prims.hip)
struct SolvePlan;    // the solve part of a level's plan (lsfm_level.hip)
struct PreLevel;     // a level prepared one level ahead (lsfm_level.hip)
struct EarlyPattern; // an early pattern build in flight (lsfm_pattern.hip)

#define LSFM_CHECK_HIP(expr)                                                                                   \
	do {                                                                                                        \
		hipError_t e__ = (expr);                                                                                \
		if (e__ != hipSuccess)                                                                                  \
			throw ::lsfm::Error{ LSFM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e__) + " at " + __FILE__ + ":" + std::to_string(__LINE__) }; \
	} while (0)
#define LSFM_FAIL(code, m) throw ::lsfm::Error{ (code), std::string(m) + " at " + __FILE__ + ":" + std::to_string(__LINE__) }
// the milliseconds between two recorded events, both complete
inline double event_ms(hipEvent_t a, hipEvent_t b)
{
	float ms = 0.0f;
	LSFM_CHECK_HIP(hipEventElapsedTime(&ms, a, b));
	return ms;
}

// bump allocator over one hipMalloc'ed slab: maps and work space of a level are carved out without any
// hipMalloc/hipFree (both synchronise) inside the timed region.
struct Arena {
	char* base = nullptr;
	size_t cap = 0, off = 0, high = 0;
	void init(size_t bytes);
	void destroy();
	void* alloc_bytes(size_t bytes);
	template <class T> T* alloc(size_t n) { return static_cast<T*>(alloc_bytes(n * sizeof(T))); }
	void reset() { off = 0; }
	size_t mark() const { return off; }
	void release(size_t m) { off = m; }
};

// Zeroes everything allocated from an arena between construction and zero(): one memset for a run of accumulators
// instead of one each (a level has ~25 of them)
struct ZeroSpan {
	Arena& ar;
	size_t from;
	explicit ZeroSpan(Arena& a) : ar(a), from((a.off + 255) & ~size_t(255)) {}
	void zero(hipStream_t s) const;
};

// One tree level's maps, flat SoA on the device.  B maps; M poses, NF features, NU U blocks, NW W blocks in total.
struct DevBatch {
	int B = 0, M = 0, NF = 0, NU = 0, NW = 0;
	// per map, host mirrors (offsets have B+1 entries)
	std::vector<int> pose_off, feat_off, u_off, w_off;
	std::vector<int> Ref, FRef, ScaP, Fix, Sign, FScaP, FFix;
	// per map, device copies of the offsets
	int *d_pose_off = nullptr, *d_feat_off = nullptr;
	// poses
	double* pose = nullptr; // [M*6]
	int* pose_id = nullptr; // [M]  = -stno
	int* pose_map = nullptr; // [M]
	int* pose_origin = nullptr; // [M] index of the local map that brought the pose (drives the elimination order)
	// features
	double* feat = nullptr; // [NF*3]
	int* feat_id = nullptr; // [NF]
	int* feat_map = nullptr; // [NF]
	// information blocks (global pose / feature indices)
	double* U = nullptr; int *Ui = nullptr, *Uj = nullptr;
	double* W = nullptr; int *photo = nullptr, *feature = nullptr;
	int* fptr = nullptr;    // [NF+1] W run of each feature
	double* V = nullptr;    // [NF*9]
	// W blocks of maps a transform passed through unchanged are not copied when the batch only feeds a join: block j of
	// such a map is W_alias[j + d_alias[map]] in the transform's INPUT (d_alias[map] == INT_MIN: materialised in W)
	const double* W_alias = nullptr;
	const int* d_alias = nullptr;
	// Mono tree levels that analyse: the sorted upper block pattern of the camera system this batch was solved with (null: not
	// kept).  The next level's pattern contains it -- a joint feature is seen by everything its sources were seen by -- so it
	// only adds what the join itself brings (PatternSeed, lsfm_join_mono.hip)
	const unsigned long long* s_keys = nullptr;
	int s_nnzb = 0;
};

struct PcgOptions { double rel_tol = 1e-12; int max_steps = 50; bool mixed = false; int spmv_variant = 0; };

// What the first run of a tree level leaves behind for the next runs of the SAME resident tree.  Everything here is
// structure: it depends on the labels, the index arrays and the join tree of the uploaded local maps, which no run
// changes -- sizes the host needs to carve the next container (the first run reads them back from the device: a
// round trip each), the block pattern of S with its hash index, the ordering / elimination structure / supernode
// groups of the factorisation (the reference redoes its symbolic analysis in every join: cholmod_analyze_p,
// Imp.cpp:2440; here it is done once per tree shape).  With a valid plan a level is enqueued without a single
// host <-> device synchronisation.
// Index arrays of a level that depend on its structure alone and that transform and join would otherwise work out again: the
// exclusive scans of the transform's kept-block flags (k_tr_flags + two scans) and the join's common-feature matches with the ranks
// of the unmatched features (hash insert + probe + a scan).  A run that analyses finds them where the level below's preparation
// one level ahead left them (schur_pattern_prefetch computes exactly these for the counts and the pattern: they were computed twice
// until round 6); a resident tree's plan keeps copies of its own (`own`).
struct LevelIndex {
	int NU = -1, NW = -1, NF = -1;             // sizes of the level's INPUT batch they belong to
	const int *KU = nullptr, *KW = nullptr;    // [NU + 2] / [NW + 2] (transform_batch)
	const int *match = nullptr, *R = nullptr;  // [NF + 1] / [NF + 2] (join_stereo_prepare)
	std::shared_ptr<IndexHold> own;            // plan-owned device memory; null: the arrays live in the preparer's arena
};
const int* level_index_keep(lsfm_context* ctx, LevelIndex& li, const int* src, size_t n); // a copy of src[0..n) in memory li owns

struct LevelPlan {
	bool valid = false;
	LevelIndex idx;
	std::vector<int> tr_cnt;     // transform: kept-block prefix values at the map boundaries (U then W)
	// Mono: sign of the new scale of every transformed map.  This one depends on VALUES (sign of a pose component): a
	// planned level compares it with what the device computes from the current values and flags the run when they differ
	std::vector<int> tr_sign;
	std::vector<int> join_rb;    // join: ranks of the unmatched features at the map boundaries
	std::vector<int> join_uo, join_wo; // Mono join: kept-U prefix at the map boundaries, W offsets of the joint maps
	std::shared_ptr<SolvePlan> solve; // pattern of S + symbolic factorisation + iteration count (lsfm_level.hip)
};

// per-run accumulators on the device, read back once at the end of a run (a warm level does not stop for them)
struct RunStatsDev {
	int chol_err;          // 1 + block column of a non-positive pivot (first one wins)
	int not_converged;     // systems left above the residual bound
	int tr_err;            // 1 + map whose transform target was not found
	int plan_stale;        // a planned level met VALUES the plan does not fit (Mono: the sign of a new scale): the run is repeated without plans
	int undone;            // systems whose refinement was enqueued with a step count from an earlier run and had not met its stopping rule when the steps ran out
	int floored;           // pivots of the separators replaced by their lower bound (static pivoting, lsfm_chol.hip k_sn_panel)
	double max_rel_residual;
	unsigned long long s_digest, factor_digest; // LSFM_FACTOR_DIGEST=1 (lsfm_stats)
	int refactor_mismatch;                      // ... systems whose second factorisation gave other bits than the first
	int s_rebuild_mismatch;                     // ... levels whose camera systems (S, E), assembled a second time from the same joint maps, were other bits
	unsigned long long k2;  // sum over the levels of sum over the features of (W run length)^2: K9's pose pairs, for its algorithmic flop count
};

// Feature-sharded joins (include/lsfm.h, lsfm_tree_set_comm): the sums that cross the GPUs.  The arrays to be reduced are
// carved out of the caller's buffer (bump allocation, restarted by every stage: a stage's arrays are consumed in stream order
// before the next stage zeroes its own), the caller's function sums them over the ranks in place.
struct Comm {
	int rank = 0, world = 1;
	lsfm_allreduce_fn fn = nullptr;
	void* user = nullptr;
	char* buf = nullptr;
	size_t cap = 0, off = 256; // (the first HDR_BYTES hold the header of the sum under way)
	// > 0: the pose-side factorisation is distributed too -- rank r owns what lies inside block r of block_maps consecutive local
	// maps of the whole tree (lsfm_tree_set_comm_blocks); 0: every rank factors everything
	int block_maps = 0;
	// Every sum is announced by a HEADER sum of 4 x int64 in the first bytes of the buffer: {ranks that failed, ranks that have not,
	// count, dtype | kind << 8} (the last two from the healthy ranks, times their number).  A healthy rank never reads it -- it
	// enqueues header and payload and goes on.  A rank whose pass threw between two sums (an error of its own: out of memory, a HIP
	// error, a buffer too small) cannot know what its peers will sum next; it FOLLOWS them instead (follow(), lsfm_prims.hip): header
	// after header it learns count and dtype of the payload, contributes zeros, and so reaches the exchange of the run's flags
	// (kind FINAL) with every collective matched -- there all ranks learn of the failure and every one of them returns an error.
	// Nobody waits for a sum the failed rank never joins (advisor, round 4).
	enum { HDR_BYTES = 256, KIND_DATA = 0, KIND_FINAL = 1 };
	bool broken = false;   // the caller's function itself failed: the communicator cannot be trusted to match anything any more
	void restart() { off = HDR_BYTES; }
	void* alloc_bytes(size_t bytes)
	{
		const size_t a = (off + 255) & ~size_t(255);
		if (a + bytes > cap)
			throw Error{ LSFM_ERR_ARG, "the buffer handed to lsfm_tree_set_comm is too small (" + std::to_string(a + bytes) + " bytes needed, " + std::to_string(cap) + " given)" };
		off = a + bytes;
		return buf + a;
	}
	template <class T> T* alloc(size_t n) { return static_cast<T*>(alloc_bytes(n * sizeof(T))); }
	// p: inside the buffer; count elements of 8 bytes (the same count on every rank)
	void allreduce(hipStream_t s, void* p, size_t count, int dtype, int kind = KIND_DATA);
	void call(hipStream_t s, size_t offset, size_t count, int dtype)
	{
		const int rc = fn(user, offset, count, dtype, (void*)s);
		if (rc) { broken = true; throw Error{ LSFM_ERR_INTERNAL, "the caller's all-reduce failed with code " + std::to_string(rc) }; }
	}
	// A rank whose pass failed: takes part in its peers' sums with zeros until they reach the exchange of the run's flags.
	// true: the peers are at that exchange (the caller now sums its flags WITHOUT a header); false: no rank is healthy any more (all
	// of them are following: nobody exchanges anything) or the communicator is broken
	bool follow(hipStream_t s);
};

// One helper thread per context for host work that the enqueuing thread need not wait for at once (the symbolic factorisation
// of the next level: lsfm_level.hip prefetch_next_level).  One job at a time; wait() returns when it is done and rethrows what
// it threw.  The thread lives as long as the context, so that what it keeps per thread (the symbolic analysis' workspace)
// is kept between jobs.
struct HostWorker {
	std::thread th;
	std::mutex m;
	std::condition_variable cv;
	std::function<void()> job;
	std::exception_ptr err;
	bool busy = false, quit = false;
	~HostWorker()
	{
		{ std::lock_guard<std::mutex> l(m); quit = true; }
		cv.notify_all();
		if (th.joinable()) th.join();
	}
	void run(std::function<void()> f)
	{
		std::unique_lock<std::mutex> l(m);
		cv.wait(l, [&] { return !busy; });
		job = std::move(f); busy = true; err = nullptr;
		if (!th.joinable())
			th = std::thread([this] {
				std::unique_lock<std::mutex> lk(m);
				for (;;)
				{
					cv.wait(lk, [&] { return quit || (busy && job); });
					if (quit) return;
					std::function<void()> j = std::move(job);
					job = nullptr;
					lk.unlock();
					std::exception_ptr e;
					try { j(); } catch (...) { e = std::current_exception(); }
					lk.lock();
					err = e; busy = false;
					cv.notify_all();
				}
			});
		cv.notify_all();
	}
	void wait()
	{
		std::unique_lock<std::mutex> l(m);
		cv.wait(l, [&] { return !busy; });
		if (err) { std::exception_ptr e = err; err = nullptr; std::rethrow_exception(e); }
	}
};

} // namespace lsfm

namespace lsfm {
// LSFM_ROCTX=1: the phases of a tree run as roctx ranges (tree run > level k > transform | join + solve; the marks of LSFM_TIMELINE as
// roctx marks), for `rocprofv3 --marker-trace --kernel-trace`.  The library is looked up at run time (librocprofiler-sdk-roctx /
// libroctx64): nothing is linked, nothing happens without the variable.
struct Roctx {
	int (*push)(const char*) = nullptr;
	int (*pop)() = nullptr;
	void (*mark)(const char*) = nullptr;
	Roctx();
};
Roctx& roctx();
struct Range {
	bool on;
	explicit Range(const char* name) : on(roctx().push != nullptr) { if (on) roctx().push(name); }
	~Range() { if (on) roctx().pop(); }
	Range(const Range&) = delete;
	Range& operator=(const Range&) = delete;
};
} // namespace lsfm

namespace lsfm {
// The events that order the three streams of a context (stream = main, stream2, stream3), one meaning each.  They live in
// lsfm_context::ord and are made with order_event_flags().  A stream waits for one through Fork or wait_for() below only; one is
// recorded by Fork, or in place where its point of the main stream lies ahead of the fork ("Streams and events", is the
// same list as a table).
enum Ord {
	evA,        // the joint maps' index arrays are complete: join_stereo_finish / join_batch_mono, main -> level_structure case 5 starts the pattern on stream2
	evB,        // the pattern of S is ready: level_structure case 4 (stream3) or 5 (stream2) -> level_structure, main, before the Schur assembly
	evC_pairs,  // feature matches and hub poses are known: join_stereo_prepare, main -> schur_pattern_early_issue starts the first half of the early pattern on stream3
	evC_runs,   // the joint run pointers are enqueued: join_stereo_prepare, main -> level_structure case 4 starts the second half of the early pattern on stream3
	evY,        // the joint maps' index arrays of the level are final: join_stereo_finish, main -> prefetch_next_level starts on stream3
	evP,        // what was prepared one level ahead is on the device: prefetch_next_level / pre_plan_complete, stream3 -> level_plan, level_structure case 3, pre_plan_complete, main
	evU,        // everything the transform's U kernel reads is final, the block kernel of the features has not begun: launch_stage, main -> k_tr_ublocks on stream2
	evG,        // the pose rows of G are complete: launch_stage, main (behind k_tr_entries) -> the U stage on stream2
	evT,        // the U stage has rejoined: launch_stage, stream2 -> launch_stage, main, before k_tr_diag
	evK9_fork,  // K9's lists and cursors are ready: launch_schur_panel, main -> the 16-slot variant on stream2
	evK9_done,  // the 16-slot variant is done: launch_schur_panel, stream2 -> launch_schur_panel, main
	evR_fork,   // the level's run pointers are final: build_schur_values, main -> k_sum_run_squares on stream2
	evR_done,   // k_sum_run_squares has read them: build_schur_values, stream2 -> run_level, main, before the next level resets arenas
	ORD_COUNT
};
} // namespace lsfm

struct lsfm_context {
	int device = 0;
	hipStream_t stream = nullptr;
	lsfm::Arena arena[3];   // rotation: level input / transformed level / joined level
	lsfm::Arena scratch;    // per-stage work space
	int cur = 0;
	size_t arena_bytes = 0, arena_req = 0; // actual size of each arena / the request it answers (may have been capped)
	lsfm::PcgOptions pcg;
	int covcols_panel = 0; // lsfm_set_covcols_panel: 0 the default of lsfm_covcols.hip, 1 plain, 2 MFMA
	// levels whose systems have at most this many poses take the one-launch dense path (lsfm_small.hip); 0: none.  The kernel holds 16;
	// the default is where it beats the level pipeline on the NC3500-like set (per-level measurements).  lsfm_set_small_solve
	int small_max = 5;
	std::string last_error;
	int* h_pinned = nullptr; // small pinned staging buffer for counters
	char* h_stage = nullptr; // pinned ring for small host->device copies: they are enqueued, not waited for
	char* d_stage = nullptr; // ... as the device sees it (null: not mapped -- copies then go through hipMemcpyAsync)
	size_t stage_size = 0, stage_off = 0;
	hipEvent_t ev_half[2] = { nullptr, nullptr }; // h2d_gather: a half of the ring may be refilled once its copy has left
	// Every entry point that resets or reallocates the arenas bumps this; a finished tree remembers the value it ended with,
	// and lsfm_tree_download refuses a result that a later call on the same context has overwritten
	unsigned long long generation = 0;
	// side stream: the pattern of S is built there while the caller's right-hand-side kernels run on the main stream (behind evA, which
	// the caller recorded and says so in SolveIO::index_arrays_at_evA); also the transform's U stage, K9's 16-slot variant and the
	// run statistics
	hipStream_t stream2 = nullptr;
	hipEvent_t ord[lsfm::ORD_COUNT] = {}; // what orders stream, stream2 and stream3: one meaning per event (lsfm::Ord)
	// Every exit that does not end with the run's events joined and the main stream synchronised (an Error caught by the run's
	// handlers or at the C ABI, the destruction of the context) calls this before arenas are reset or freed: waits for stream2 and
	// stream3, swallows and clears what they report.  Host only; twice is as good as once; the helper thread and `pre` are not its business
	void quiesce_side_streams();
	// Early pattern of S (Stereo tree levels that analyse): the pose pairs of the JOINT map follow from the level's input index
	// arrays, the feature matches and the hub pose of every transformed map, all known before the transform's heavy kernels
	// run -- the pattern is put together on the side stream while those run, and the host's symbolic analysis no longer
	// waits for them (lsfm_pattern.hip: schur_pattern_early_*).  The level's input and the hub list reach the join through the
	// transform's hook (join_stereo_prepare).
	std::shared_ptr<lsfm::EarlyPattern> early; // the build in flight (null: none)
	hipStream_t stream3 = nullptr;      // its own stream: the side stream carries the transform's U stage, which waits for the block kernel
	// One level ahead (Stereo tree runs that analyse): while the device factors and refines level L, the pattern of level
	// L + 1's system is put together on stream3 from level L's joint maps (their index arrays are final long before the
	// solve ends) and the host analyses it -- level L + 1 then finds its pattern and its symbolic factorisation waiting
	// (lsfm_level.hip: prefetch_next_level).  Their arrays live in two small arenas used in turn.
	lsfm::Arena sarena[2];
	// what was prepared for the level about to run (null: nothing).  Its symbolic factorisation (host work) may still be under way on
	// the helper thread when the level starts; releasing the object waits for it -- nothing the thread reads goes before (~PreLevel)
	std::shared_ptr<lsfm::PreLevel> pre;
	// ... and, when an earlier run of the tree has left the refinement step count of that level, everything else the level
	// would stop for (kept-block counts of its transform, unmatched-feature ranks of its join): a plan of the level made
	// one level ahead -- the level then runs like a planned one, without a single host <-> device round trip: its transform, join
	// and Schur assembly are enqueued while the helper thread works, solve_batch completes the plan (lsfm_level.hip)
	lsfm::LevelPlan pre_plan;
	int pre_plan_level = -1;
	std::unique_ptr<lsfm::HostWorker> worker;
	void drop_prepared() { pre.reset(); pre_plan = lsfm::LevelPlan(); pre_plan_level = -1; }
	double dbg_gap_ms = 0.0; // (LSFM_LEVEL_GAPS=1: from the event behind a level's solve to the next level's first, summed over a run)
	// LSFM_TIMELINE=1: host wall-clock marks of a tree run (where the enqueuing thread is when), printed at the end of the run
	std::vector<std::pair<const char*, double>> timeline;
	bool timeline_on = false;
	void mark(const char* what);
	bool in_tree_run = false;
	lsfm_stats* stats = nullptr; // optional sink during a tree run
	lsfm::LevelPlan* plan = nullptr; // plan of the tree level being run (null: stage-level calls, nothing is recorded or reused)
	bool warm() const { return plan && plan->valid; }
	lsfm::RunStatsDev* d_run = nullptr; // device accumulators of the current run
	lsfm::Comm* comm = nullptr;         // feature-sharded tree run (set for the duration of lsfm_tree_run): sums cross the GPUs
	// timing of stages without stopping for them: events from a pool, elapsed times added to their sinks by flush_times()
	std::vector<hipEvent_t> ev_pool;
	size_t ev_next = 0;
	struct Timed { hipEvent_t a, b; double* sink; };
	std::vector<Timed> timed;
	hipEvent_t pool_event();
	void defer_time(hipEvent_t a, hipEvent_t b, double* sink) { timed.push_back(Timed{ a, b, sink }); }
	void flush_times(); // after the stream has been synchronised
	// bytes_each: an upper bound of what a call may need (the estimates ignore that joins merge their common features: an order of
	// magnitude at depth).  start_small: allocate an eighth of it and let grow_arenas() double it when a run exhausts an arena --
	// a cold process paid 2.5-3 s of hipMalloc for the 4 x 26 GB the NC3500-like estimate asks for, of which a run touches 3 GB
	void ensure_arenas(size_t bytes_each, bool start_small = false);
	bool grow_arenas(); // false: already at the bound
	bool arena_small = false;
	size_t arena_bound = 0; // what the arenas may grow to (the capped request)
};

namespace lsfm {

// "This stretch runs on another stream (and allocates from another arena)": until the end of the scope -- however it is left --
// ctx->stream names `other` (and ctx->scratch names `arena`), so everything called inside enqueues and allocates there.
struct OnStream {
	lsfm_context* c; hipStream_t& s; Arena* a;
	OnStream(lsfm_context* ctx, hipStream_t& other, Arena* arena = nullptr) : c(ctx), s(other), a(arena) { std::swap(c->stream, s); if (a) std::swap(c->scratch, *a); }
	~OnStream() { if (a) std::swap(c->scratch, *a); std::swap(c->stream, s); }
	OnStream(const OnStream&) = delete;
	OnStream& operator=(const OnStream&) = delete;
};
// "The main stream waits / a side stream starts behind a point someone recorded": the one place besides Fork that makes a stream wait
inline void wait_for(lsfm_context* ctx, hipStream_t s, Ord e) { LSFM_CHECK_HIP(hipStreamWaitEvent(s, ctx->ord[e], 0)); }
// "This stretch runs on a side stream, beside the main stream": an OnStream scope whose side stream starts behind `start` -- recorded
// here on the main stream, or (record = false) by someone else before; without a start, nothing the stretch reads comes from the main
// stream.  join(e) records e behind the stretch and makes the main stream wait for it; done(e) only records it, for a wait_for()
// elsewhere (the prefetch rejoins the NEXT level).  A scope left without either enqueues nothing more: the stretch is followed on its
// stream by one that joins -- or an exception is passing, and the handlers wait for the side streams (quiesce_side_streams).
// Inside the scope ctx->stream names the side stream and `side` the main one, as with OnStream.
struct Fork {
	lsfm_context* c; hipStream_t main; OnStream on;
	Fork(lsfm_context* ctx, hipStream_t& side, Arena* arena = nullptr) : c(ctx), main(ctx->stream), on(ctx, side, arena) {}
	Fork(lsfm_context* ctx, hipStream_t& side, Ord start, bool record = true, Arena* arena = nullptr) : Fork(ctx, side, arena)
	{
		if (record) LSFM_CHECK_HIP(hipEventRecord(c->ord[start], main));
		wait_for(c, c->stream, start);
	}
	void done(Ord e) { LSFM_CHECK_HIP(hipEventRecord(c->ord[e], c->stream)); }
	void join(Ord e) { done(e); wait_for(c, main, e); }
};

// ---- primitives (lsfm_prims.hip; rocPRIM scan / radix sort on the context stream) ------------------------
void dev_exclusive_scan(lsfm_context* ctx, const int* in, int* out, size_t n); // out[n] = total (n+1 entries written)
void dev_sort_pairs_u64(lsfm_context* ctx, unsigned long long* keys, int* vals, size_t n, int end_bit, int begin_bit = 0); // stable, bits [begin, end)
void dev_sort_keys_u64(lsfm_context* ctx, const unsigned long long* keys, unsigned long long* sorted, size_t n, int begin_bit, int end_bit);
int d2h_int(lsfm_context* ctx, const int* dptr);
void d2h_ints(lsfm_context* ctx, const int* dptr, int* h, size_t n);
void h2d(lsfm_context* ctx, void* d, const void* h, size_t bytes);
// many host pieces -> ONE contiguous device range, in order, streamed through the two halves of the pinned ring (the host
// fills one half while the other one is on the wire): a set of N local maps arrives as a dozen large copies instead of
// ~3 N pageable ones.  Synchronises before and after.
struct HostPiece { const void* p; size_t bytes; };
void h2d_gather(lsfm_context* ctx, void* d, const std::vector<HostPiece>& pieces);
// Several small copies of a stage as ONE staged transfer + ONE kernel: a level makes ~20 of them (map records, offsets, copies
// of label arrays), each a 10 us blit of its own when issued one by one -- 320 per tree, 3.4 ms of the NC3500-like tree's 41.
// Host pieces are packed into the pinned ring behind a table of (destination, source, bytes), the whole goes to the device in
// one copy, k_copy_many moves every piece (device-to-device pieces straight from their source).  Sizes are multiples of 4.
struct CopyBatch {
	lsfm_context* ctx;
	struct Item { void* dst; const void* src; size_t bytes; bool host; };
	std::vector<Item> items;
	explicit CopyBatch(lsfm_context* c) : ctx(c) {}
	void h2d(void* d, const void* h, size_t bytes) { if (bytes) items.push_back(Item{ d, h, bytes, true }); }
	void d2d(void* d, const void* s, size_t bytes) { if (bytes) items.push_back(Item{ d, s, bytes, false }); }
	void flush(); // enqueues on ctx->stream; the host sources may be freed afterwards
};
void d2h(lsfm_context* ctx, void* h, const void* d, size_t bytes);
void dev_zero(lsfm_context* ctx, void* d, size_t bytes);
void fill_async(hipStream_t s, void* d, int byte, size_t bytes); // (a kernel of the library, not hipMemsetAsync: lsfm_prims.hip)

// ---- batches (lsfm_batch.hip) -------------------------------------------------------------------------------
void batch_upload(lsfm_context* ctx, Arena& ar, const lsfm_map* maps, int N, bool mono, DevBatch& out);
void batch_download_map(lsfm_context* ctx, const DevBatch& b, int k, bool mono, lsfm_map* out);
// map_alloc (lsfm_map.hpp: the allocator of every map the library hands out) for an entry point: the map, or an Error (LSFM_ERR_OOM)
inline void map_new(lsfm_map& g, const lsfm_map* like, int m, int n, int nU, int nW, bool pose_origin)
{
	if (map_alloc(g, like, m, n, nU, nW, pose_origin) != LSFM_OK) throw Error{ LSFM_ERR_OOM, "out of host memory for the merged map" };
}
struct CopyBatch;
// uploads pose_off / feat_off, fills pose_map / feat_map (cb != null: the uploads join the caller's batch, which then calls batch_fill_maps)
void batch_set_offsets(lsfm_context* ctx, Arena& ar, DevBatch& b, CopyBatch* cb = nullptr);
void batch_fill_maps(lsfm_context* ctx, DevBatch& b);
// A map packed into one contiguous device buffer for the hand-off between GPUs (include/lsfm.h): header, then the arrays
// with map-local indices, each 256-byte aligned.
struct PackHeader {
	int magic, version, mono, m, n, nU, nW, Ref, FRef, ScaP, Fix, Sign, FScaP, FFix, pad0, pad1;
	unsigned long long total;
	unsigned long long off[12]; // pose feat U W V | pose_id pose_origin feat_id Ui Uj photo fptr
	unsigned long long pad[11];
};
static_assert(sizeof(PackHeader) == 256, "the header is the first 256 bytes of a pack");
#define LSFM_PACK_MAGIC 0x4d46534c
size_t pack_layout(PackHeader& h); // fills off[] and total from the counts
void batch_pack_map(lsfm_context* ctx, const DevBatch& b, int k, bool mono, void* dst, size_t cap);
// the single map of `b` cut by feature label: slice g holds the features with feat_id % nslices == g (order kept) with their V
// and W blocks, and ALL poses and U blocks.  batch_slice_counts: features / W blocks of every slice (synchronises).
void batch_slice_counts(lsfm_context* ctx, const DevBatch& b, int nslices, std::vector<int>& nf, std::vector<int>& nw);
void batch_pack_slice(lsfm_context* ctx, const DevBatch& b, bool mono, int nslices, int slice, int nf, int nw, void* dst, size_t cap);
void batch_unpack_maps(lsfm_context* ctx, Arena& ar, const void* const* packed, const PackHeader* hdr, int N, bool mono, DevBatch& out);
// digest of everything a tree's plans are derived from: labels, index arrays, pose origins (synchronises)
unsigned long long batch_structure_digest(lsfm_context* ctx, const DevBatch& b);

// ---- transform (lsfm_transform.hip): K1-K4 ------------------------------------------------------------------
// target_ref[b] < 0 ... map b is passed through unchanged; otherwise the pose id the map is re-expressed in
// (Mono: target_scap / target_fix as well).  out is allocated from `ar`.
// level_targets: those of a tree level's transform, whose maps (2i, 2i + 1) = (End, Cur) are joined next: an odd output of the
// level below goes back to its first frame and End is expressed in Cur's frame; a map already in its target frame is passed
// through (map_in_frame).  Returns the transforms the reference counts (those included).  The level's own transform and the
// preparation one level ahead (prefetch_next_level, on the joint maps) both take it from here.
inline bool map_in_frame(const DevBatch& X, int b, int tref, int tscap, bool mono) { return X.Ref[b] == tref && (!mono || X.ScaP[b] == tscap); } // Imp.cpp:352 / 3176
int level_targets(const DevBatch& X, bool mono, std::vector<int>& tref, std::vector<int>& tscap, std::vector<int>& tfix);
// Where the transform's W stage writes when its consumer has already laid out the next container (a join): the run of
// input feature f starts at wbase[f] of W / photo / feature, blocks are labelled newf[f], srcf[] records the input feature.
struct TrRedirect {
	const int* wbase = nullptr;
	const int* newf = nullptr;
	double* W = nullptr;
	int *photo = nullptr, *feature = nullptr, *srcf = nullptr;
};
// hook: called once everything of `out` except the information blocks exists (poses, feature values, V', run pointers,
// offsets); its answer redirects the W blocks.  hub: [B] global pose index of the hub column of every transformed map, -1: passed
// through (Stereo; null: Mono, or a batch without poses) -- with the transform's input, what the early pattern of S is made from.
// keep_scratch: the caller releases the scratch arena (allocations made in the hook outlive the call).
using TrHook = std::function<TrRedirect(DevBatch& mid, const int* hub)>;
void transform_batch(lsfm_context* ctx, Arena& ar, const DevBatch& in, const std::vector<int>& target_ref,
                     const std::vector<int>& target_scap, const std::vector<int>& target_fix, bool mono, DevBatch& out,
                     bool alias_passthrough = false, const TrHook* hook = nullptr);

// ---- join + solve (lsfm_join.hip, lsfm_pattern.hip, lsfm_solve.hip): K5-K11 ---------------------------------------------------
struct JoinWork; // device work arrays shared between assembly and solve
struct SolveIO {
	// system of `nseg` independent camera systems laid out back to back (block rows = poses of the batch)
	int M = 0, NF = 0, NU = 0, NW = 0, nseg = 0;
	const int* d_pose_seg = nullptr;   // [M] segment of each pose
	const int* d_feat_seg = nullptr;   // [NF]
	const unsigned char* d_seg_active = nullptr; // [nseg] 0 = carried map: state is not touched
	const double* U = nullptr; const int *Ui = nullptr, *Uj = nullptr;
	const double* W = nullptr; const int *photo = nullptr, *fptr = nullptr;
	const double* V = nullptr;
	const double* ea = nullptr;        // [M*6]
	const double* eb = nullptr;        // [NF*3]
	const double* x0 = nullptr;        // [M*6] initial guess (may be null -> zero)
	const unsigned char* d_fixed = nullptr; // [M*6] optional: 1 = scalar removed from the system (Mono gauge)
	const int* d_pose_origin = nullptr;     // [M] optional: index of the local map that brought the pose (null: its position)
	double* x_pose = nullptr;          // [M*6] out
	double* x_feat = nullptr;          // [NF*3] out
	std::vector<int> seg_rows;         // host: block rows per segment
	// optional: [nseg + 1] first pose / feature / U block of every segment (segments are contiguous ranges of the batch).  With them,
	// a level whose systems have at most 16 poses is solved by the one-launch dense path (lsfm_small.hip)
	const int *d_pose_off = nullptr, *d_feat_off = nullptr, *d_u_off = nullptr;
	// optional (Stereo tree levels on the sparse pipeline): the W part of the right-hand sides is left to the Schur assembly -- ea
	// holds U's part only, eb the V part (lsfm_solve.hpp RhsFused; null: ea / eb are complete)
	const struct RhsFused* rhs = nullptr;
	// optional (Mono tree levels that analyse): the pattern of S follows from the pattern of the level below instead of being built
	// from every pose pair of every feature again (lsfm_solve.hpp PatternSeed; null: from scratch)
	const struct PatternSeed* seed = nullptr;
	// the caller recorded evA where the joint map's index arrays were complete and went on to enqueue its right-hand-side kernels:
	// a level that analyses may build the pattern of S on the side stream from there (level_structure, case 5)
	bool index_arrays_at_evA = false;
	// refinement steps: > 0 = what an earlier run of this tree needed at this level (the steps are then enqueued without asking the
	// device after each one; whether they sufficed is read at the end of the run -- lsfm_tree_run: errors of a level may be left in
	// d_run and read there)
	int step_hint = 0;
	// the caller waits for the device behind the solve anyway (a Mono level that analyses): a hinted refinement may ask once
	bool caller_syncs = false;
};
struct SolveOutcome {
	int not_converged = 0;                    // systems left above their bound (0 where the outcome stays in the run's device record)
	int steps_used = 0;                       // refinement steps a solve that asked after each one needed; 0: the steps were planned
	const unsigned long long* keys = nullptr; // sorted upper pattern of the system just solved (scratch arena: valid until the caller releases it); null: the dense path leaves none
	int nnzb = 0;
	hipEvent_t end = nullptr;                 // recorded behind the back-substitution
};
// Does a level whose largest system has most_rows poses take the one-launch dense path?  16-row strips of its panel; 0: no (the
// systems are too large -- lsfm_context::small_max --, or the run is feature-sharded or in mixed precision).  The ONE place that
// decides it: the join (offsets, fused right-hand sides, early pattern), the preparation one level ahead and the solve must agree
int small_level_strips(const lsfm_context* ctx, int most_rows);
inline int most_rows(const std::vector<int>& seg_rows) { int most = 0; for (int r : seg_rows) most = r > most ? r : most; return most; }
inline int small_level_strips(const lsfm_context* ctx, const std::vector<int>& seg_rows) { return small_level_strips(ctx, most_rows(seg_rows)); }
// the join of such a level (io.seg_rows set): the ranges of its joins in the joint maps `out`, by which the dense path walks them, to io
void small_level_offsets(lsfm_context* ctx, const DevBatch& out, SolveIO& io);
void small_solve_launch(lsfm_context* ctx, const SolveIO& io, int strips, int* status, double* max_rel);
// lsfm_selftest_small: G systems back to back in h (the batch's numbering), one small_solve_launch; x_pose / x_feat go in as the prefill
struct HostSystem;
int small_selftest(lsfm_context* ctx, int G, const int* pose_off, const int* feat_off, const int* u_off, const unsigned char* active, const HostSystem& h,
                   const unsigned char* fixed, int strips, double* x_pose, double* x_feat, int* status, double* max_rel);
SolveOutcome solve_batch(lsfm_context* ctx, const SolveIO& io);
// groups: consecutive maps (2g, 2g+1) of `in` are joined, a trailing unpaired map is carried over unchanged.
// Produces `out` (ceil(B/2) maps) with the solved state.  eP_out / eF_out (host, optional) receive the right-hand
// sides of group 0 when B <= 2 (stage-level C ABI).  step_hint: SolveIO::step_hint of the join's solve, whose outcome is returned
// (systems left above their bound are counted into ctx->stats here).
SolveOutcome join_batch_stereo(lsfm_context* ctx, Arena& ar, const DevBatch& in, DevBatch& out, double* eP_out, double* eF_out, int step_hint = 0);
SolveOutcome join_batch_mono(lsfm_context* ctx, Arena& ar, const DevBatch& in, DevBatch& out, double* eP_out, double* eF_out, int step_hint = 0);
// Gauss-Newton polish of the map-joining objective over all local maps at once (lsfm_gn.hip, shared declarations
// lsfm_gn.hpp: structure lsfm_gn_structure.cpp, one assembly lsfm_gn_assemble.hip, chi^2 and weights lsfm_gn_chi2.hip; C ABI: lsfm_gn_polish)
int gn_polish(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, lsfm_map* x, int iters, int kind, double c, double* obj, double* gnorm,
              int* halvings, double* chi2, double* weight);
// per-feature chi^2 c_kf of every local feature instance at a global state and the Gauss-Newton polish that down-weights single
// features by an M-estimator on c_kf / 3 (lsfm_gn.hip, kernels lsfm_gn_chi2.hip; C ABI: lsfm_map_feature_chi2, lsfm_gn_polish_robust_features)
int map_feature_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, double* fchi2, double* pose_chi2);
int gn_polish_features(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, lsfm_map* x, int iters, int kind, double c, double* obj, double* gnorm,
                       int* halvings, double* fchi2, double* fweight);
// per-map chi^2 of the map-joining objective at a global state (lsfm_gn.hip, kernel lsfm_gn_chi2.hip; C ABI: lsfm_map_chi2)
int map_chi2(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, double* chi2, int* dof);
// the joint system of the local maps linearised at x as a map of its own, every block once (lsfm_gn.hip; C ABI: lsfm_gn_linearise;
// with fweight, [sum n_k] weights in [0, 1] of the features' conditional terms: lsfm_gn_linearise_features).
// times (may be null): [3] ms of the assembly, the W and the U coalescing launch -- with fweight [4], the chi^2 pass + slot fill ahead of
// them; counts (may be null): [4] NWJ, nW', NUJ, nU'
int gn_linearise(lsfm_context* ctx, const lsfm_map* maps, int N, bool mono, const lsfm_map* x, const double* weight, const double* fweight,
                 lsfm_map* out, double* obj, double* b, double* times, int* counts);
// marginal covariances of a map's information matrix (lsfm_cov.hip; C ABI: lsfm_map_covariance).  times (may be null): [4] ms of the
// Schur reduction + analysis, the factorisation, the selected inversion + pose gather, the feature part
int map_covariance(lsfm_context* ctx, const lsfm_map* map, bool mono, double* pose_cov, double* feat_cov, double* pair_cov, int cap_blocks, int* nnzb,
                   double* times);
// whole columns of Sigma for the poses poses[k], solved side by side against the same factor and refined in fp64 (lsfm_covcols.hip; C ABI:
// lsfm_map_covariance_columns).  times (may be null): [4] ms of reduce + analyse, factorisation, all sweeps and products, the feature part
int map_covariance_columns(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* poses, int k, double* pose_cols, double* feat_cols, double* joint,
                           int* steps, double* last_corr, double* times);
// whole columns of Sigma for the features feats[k] and the gate d^2 = dx^T Var(x_f - x_g)^-1 dx of the K feature pairs pairs[2 K], three
// columns per feature or pair through the same sweeps and refinement (lsfm_featcols.hip; C ABI: lsfm_map_covariance_feature_columns,
// lsfm_map_feature_pair_gate).  times (may be null): [4] ms of reduce + analyse, factorisation, all sweeps and products, the feature part / the gate kernel
int map_covariance_feature_columns(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* feats, int k, double* pose_cols, double* feat_cols,
                                   double* joint, int* steps, double* last_corr, double* times);
int map_feature_pair_gate(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* pairs, int K, double* d2, double* cov_diff, int* steps,
                          double* last_corr, double* times);
// the sequential joint-compatibility selection among the K feature pairs pairs[2 K] (lsfm_jointgate.hip; C ABI:
// lsfm_map_feature_pair_joint_gate, lsfm_selftest_pair_select).  times (may be null): [6] ms of reduce + analyse, factorisation, sweeps +
// refinement, the blocks of C, the selection's kernels, the downloads with the selection's host preparation and allocations
int map_feature_pair_joint_gate(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* pairs, int K, const int* order, double tau, int* status,
                                double* delta, double* d2, double* joint_C, int* accepted, int* implied, double* D2, int* steps, double* last_corr, double* times);
int pair_select_selftest(lsfm_context* ctx, int K, const double* C, const double* d, const int* ends, const int* order, double tau, int* status, double* delta,
                         double* D2, int* accepted, int* implied);
// the map with the K feature pairs pairs[2 K] declared equal, and the joint compatibility D^2 of all of them (lsfm_merge.hip, structure
// lsfm_merge_structure.cpp; C ABI: lsfm_map_merge_features).  times (may be null): [5] ms of upload + W' / V' passes + the merged map's way
// to the host, its upload + reduction + analysis + factorisation, right-hand side + sweeps + refinement, back-substitution + D^2, download
int map_merge_features(lsfm_context* ctx, const lsfm_map* map, bool mono, const int* pairs, int K, lsfm_map* out, double* d2, int* dof, int* rep,
                       int* steps, double* last_corr, double* times);
// every feature pair within `radius` whose bound q = 1/2 d^T (Sigma_ff + Sigma_gg)^-1 d <= tau (feat_cov may be null: the radius alone), by a
// cell search (lsfm_candidates.hip; C ABI: lsfm_map_feature_pair_candidates).  *count is set before a cap that is too small is refused.
// times (may be null): [4] ms of upload + keys, sort + cell table, count + scan, fill + sort + download; info (may be null): [4] cells,
// fullest cell, pair tests, candidates
int map_feature_pair_candidates(lsfm_context* ctx, const lsfm_map* map, const double* feat_cov, double radius, double tau, int* pairs, double* dist2, double* q,
                                long long cap, long long* count, double* times, long long* info);
// the two feature-side pieces of the solve on their own (lsfm_solve.hip; C ABI: lsfm_inverse_v / lsfm_solve_features); host pointers,
// arguments checked by the caller
int inverse_v(lsfm_context* ctx, double* V, int n);
int vinv_selftest(lsfm_context* ctx, const double* V, const double* eb, int n, int skip, double* IV, double* LY); // C ABI: lsfm_selftest_vinv
int solve_features(lsfm_context* ctx, const double* W, const double* IV, const double* eb, const double* dpa, double* dpb, int m, int n, const int* mapCor,
                   const int* photo);
bool no_timing_events(); // (LSFM_NO_TIMING_EVENTS=1: the phase brackets are not recorded -- the stage times of lsfm_stats stay zero)
#define LSFM_REC_T(e, s) do { if (!lsfm::no_timing_events()) LSFM_CHECK_HIP(hipEventRecord(e, s)); } while (0)
unsigned timing_event_flags(); // (lsfm_prims.hip: events without the system-scope fence)
unsigned order_event_flags();
// level_keys / level_nnzb: SolveOutcome::keys / nnzb of the level whose joint maps Y are (the one being solved)
void prefetch_next_level(lsfm_context* ctx, const DevBatch& Y, const std::vector<int>& target_ref, int next_level, int step_hint,
                         const unsigned long long* level_keys, int level_nnzb);
int spmv_external(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const double* x, double* y, int reps,
                  double* avg_ms, double* bytes);
// the device Cholesky on a caller's matrix, without refinement (lsfm_chol.hip; C ABI: lsfm_selftest_chol); arguments checked by the caller
int chol_selftest(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                  const int* pose_seg, int nseg, const double* r, int nrhs, int mode, double* z, double* dot, int* perm, int* colptr, int* rowidx,
                  double* L, double* Dinv, double* dscale, int cap_blocks, int* info);
// the side-by-side sweeps of the columns calls on a caller's matrix, without refinement, and one residual product (lsfm_covcols.hip;
// C ABI: lsfm_selftest_cc_sweeps); arguments checked by the caller
int cc_sweeps_selftest(lsfm_context* ctx, int m, const int* rowptr, const int* colidx, const double* val, const int* origin, const unsigned char* fixed,
                       const double* B, int R, const double* X, double* x, double* fwd, int* perm, double* dscale, double* y, int* info);

int wstream_bench(lsfm_context* ctx, long long nblocks, int mode, int reps, double* avg_ms); // measurement: W access patterns vs stream copy
// fills, word copies and CopyBatch against a host mirror (lsfm_prims.hip; C ABI: lsfm_selftest_prims)
int prims_selftest(lsfm_context* ctx, int cases, unsigned seed);
} // namespace lsfm
