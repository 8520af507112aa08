// The tree scheduler (lsfm_tree.hpp): one level, one pass over the tree, and the run that repeats a pass where it has to.
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "lsfm_join.hpp"
#include "lsfm_tree.hpp"

namespace lsfm {

namespace {

// the plan level `level` runs with (ctx->plan; null: none).  true: this run does the level's symbolic work (it may have done it one
// level ahead)
bool level_plan(lsfm_context* ctx, lsfm_tree* t, int level)
{
	ctx->plan = (t->use_plans && level < (int)t->plans.size()) ? &t->plans[level] : nullptr;
	const bool analysing = !(ctx->plan && ctx->plan->valid);
	if (!ctx->plan && !t->mono && ctx->pre_plan.valid && ctx->pre_plan_level == level)
	{
		// ... all of it: the plan of this level was made while the level below was being solved (prefetch_next_level)
		ctx->plan = &ctx->pre_plan;
		wait_for(ctx, ctx->stream, evP);
	}
	return analysing;
}

// LSFM_LEVEL_GAPS=1: what the device waited for the host between the levels of a run (the event behind a level's solve was
// handed over long before the host got here; this one is stamped when the stream reaches it, or when it arrives)
void level_gap(lsfm_context* ctx, hipEvent_t prev_solve_end, hipEvent_t level_begin)
{
	static const bool gaps = getenv("LSFM_LEVEL_GAPS") != nullptr;
	if (gaps && prev_solve_end) ctx->defer_time(prev_solve_end, level_begin, &ctx->dbg_gap_ms);
}

// one level: transform the maps that need it, then join the pairs.  prev_solve_end: the event behind the solve of the level below
// (null: none); inject_level: tests -- the level in which this rank's pass fails (LSFM_TEST_FAIL_RANK), -1: none.  Returns the event
// behind this level's solve
hipEvent_t run_level(lsfm_context* ctx, lsfm_tree* t, lsfm_stats* st, int level, hipEvent_t prev_solve_end, int inject_level)
{
	const bool analysing = level_plan(ctx, t, level);
	char rname[48];
	snprintf(rname, sizeof rname, "lsfm level %d (%d maps)", level, t->level.B);
	Range rlevel(rname);
	ctx->mark("level");
	if ((int)t->step_hint.size() <= level) t->step_hint.resize(level + 1, 0);
	// what an earlier run of this tree needed here (0: nothing known; SolveIO::step_hint)
	const int step_hint = t->step_hint[level];
	DevBatch& X = t->level;
	const int npairs = X.B / 2;
	std::vector<int> tref, tscap, tfix;
	const int ntr = level_targets(X, t->mono, tref, tscap, tfix);
	// stage times from events on the stream (a warm level is only enqueued: host clocks say nothing about it)
	hipEvent_t e_t0 = ctx->pool_event(), e_t1 = ctx->pool_event(), e_t2 = ctx->pool_event();
	LSFM_REC_T(e_t0, ctx->stream);
	level_gap(ctx, prev_solve_end, e_t0);
	// three arenas in rotation: X (this level; slot -1 = the resident inputs, never written) stays alive until the join
	// is done, because the W blocks of the maps the transform passes through are read from X, not copied (W_alias)
	const int so = t->slot < 0 ? 0 : (t->slot + 1) % 3, sm = t->slot < 0 ? 1 : (t->slot + 2) % 3;
	Arena& other = ctx->arena[so];
	Arena& mine = ctx->arena[sm];
	// (the run statistics of the level below read its run pointers on stream2: long done, but nothing else says so)
	wait_for(ctx, ctx->stream, evR_done);
	other.reset();
	mine.reset();
	DevBatch Xt, Y;
	SolveOutcome oc;
	// tests (tests/test_gpu_sharded.py): ONE rank of a feature-sharded run fails in the middle of a level, between two sums
	const bool inject = inject_level == level;
	if (t->mono)
	{
		{ Range r("lsfm transform"); transform_batch(ctx, other, X, tref, tscap, tfix, true, Xt, true); }
		if (inject) LSFM_FAIL(LSFM_ERR_INTERNAL, "injected failure of this rank (LSFM_TEST_FAIL_RANK)");
		LSFM_REC_T(e_t1, ctx->stream);
		Range r("lsfm join + solve");
		oc = join_batch_mono(ctx, mine, Xt, Y, nullptr, nullptr, step_hint);
	}
	else
	{
		// Stereo: the joint map is laid out in the middle of the transform (labels, V' and run lengths are known before the
		// W stage), and the transform's block kernel writes every W' block straight to its place in the joint map
		JoinState js;
		const size_t smark = ctx->scratch.mark();
		TrHook hook = [&](DevBatch& mid, const int* hub) {
			join_stereo_prepare(ctx, mine, mid, Y, js, &X, hub);
			TrRedirect rd;
			rd.wbase = js.wbase; rd.newf = js.newf; rd.W = Y.W; rd.photo = Y.photo; rd.feature = Y.feature; rd.srcf = js.srcf;
			return rd;
		};
		{ Range r("lsfm transform"); transform_batch(ctx, other, X, tref, tscap, tfix, false, Xt, false, &hook); } // (the join's layout kernels run inside)
		if (inject) LSFM_FAIL(LSFM_ERR_INTERNAL, "injected failure of this rank (LSFM_TEST_FAIL_RANK)");
		LSFM_REC_T(e_t1, ctx->stream);
		Range r("lsfm join + solve");
		js.smark = smark; // everything of this level goes at once
		oc = join_stereo_finish(ctx, Xt, Y, js, nullptr, nullptr, step_hint);
		ctx->pre_plan = LevelPlan(); // (consumed, if it was this level's)
		ctx->pre_plan_level = -1;
		if (analysing && Y.B > 1 && !ctx->comm)
		{
			// while the device solves this level: the next level's pattern and symbolic factorisation (lsfm_level.hip)
			std::vector<int> nref, nscap, nfix;
			level_targets(Y, false, nref, nscap, nfix);
			prefetch_next_level(ctx, Y, nref, level + 1, level + 1 < (int)t->step_hint.size() ? t->step_hint[level + 1] : 0, oc.keys, oc.nnzb);
		}
		else ctx->drop_prepared();
	}
	LSFM_REC_T(e_t2, ctx->stream);
	if (oc.steps_used > 0) t->step_hint[level] = oc.steps_used;
	ctx->plan = nullptr;
	t->level = Y;
	t->slot = sm;
	if (st)
	{
		ctx->defer_time(e_t0, e_t1, &st->t_transform_ms);
		ctx->defer_time(e_t1, e_t2, &st->t_join_ms);
		st->levels++; st->joins += npairs; st->transforms += ntr;
	}
	return oc.end;
}

// one pass over the tree; with valid plans nothing in here waits for the device before the final synchronisation
void tree_pass(lsfm_context* ctx, lsfm_tree* t, lsfm_stats* st, int inject_level)
{
	Range rrun("lsfm tree run");
	// level 0 reads the resident inputs where they are (no level writes its input), so a tree can be run repeatedly
	t->slot = -1;
	t->done = false;
	ctx->generation++;
	ctx->arena[0].reset(); ctx->arena[1].reset(); ctx->arena[2].reset(); ctx->scratch.reset();
	ctx->stage_off = 0; // the stream is idle: the staging ring starts over
	ctx->drop_prepared(); ctx->early.reset(); // nothing prepared by an earlier run
	LSFM_CHECK_HIP(hipMemsetAsync(ctx->d_run, 0, sizeof(RunStatsDev), ctx->stream));
	static const bool poison = getenv("LSFM_POISON") != nullptr; // debug: every byte a run has not written itself reads as NaN / -1
	if (poison)
	{
		for (int i = 0; i < 3; i++) LSFM_CHECK_HIP(hipMemsetAsync(ctx->arena[i].base, 0xFF, ctx->arena[i].cap, ctx->stream));
		LSFM_CHECK_HIP(hipMemsetAsync(ctx->scratch.base, 0xFF, ctx->scratch.cap, ctx->stream));
		for (int i = 0; i < 2; i++) if (ctx->sarena[i].base) LSFM_CHECK_HIP(hipMemsetAsync(ctx->sarena[i].base, 0xFF, ctx->sarena[i].cap, ctx->stream));
	}
	t->level = t->input;
	const int nlev = tree_levels(t->N);
	if ((int)t->plans.size() != nlev + 1) t->plans.assign(nlev + 1, LevelPlan());
	int level = 0;
	hipEvent_t solve_end = nullptr; // behind the solve of the level just run (LSFM_LEVEL_GAPS)
	for (; t->level.B > 1 && (t->stop_level <= 0 || level < t->stop_level); level++) solve_end = run_level(ctx, t, st, level, solve_end, inject_level);
	// final map back to its first frame (Imp.cpp:2039-2063 / 6613-6630)
	DevBatch& X = t->level;
	if (t->final_reanchor && X.B == 1 && X.Ref[0] > X.FRef[0])
	{
		std::vector<int> tref(1, X.FRef[0]), tscap(1, X.FScaP[0]), tfix(1, X.FFix[0]);
		const int so = t->slot < 0 ? 0 : (t->slot + 1) % 3;
		Arena& other = ctx->arena[so];
		other.reset();
		DevBatch Xt;
		hipEvent_t e0 = ctx->pool_event(), e1 = ctx->pool_event();
		LSFM_REC_T(e0, ctx->stream);
		ctx->plan = t->use_plans ? &t->plans[nlev] : nullptr;
		transform_batch(ctx, other, X, tref, tscap, tfix, t->mono, Xt);
		if (ctx->plan) ctx->plan->valid = true;
		ctx->plan = nullptr;
		LSFM_REC_T(e1, ctx->stream);
		ctx->defer_time(e0, e1, &st->t_transform_ms);
		st->transforms++;
		t->level = Xt;
		t->slot = so;
	}
	LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
}

// tests (tests/test_gpu_sharded.py): what to make go wrong in this attempt of a feature-sharded run.  LSFM_TEST_FAIL_RANK=r makes rank
// r's FIRST attempt fail -- LSFM_TEST_FAIL_KIND=throw (default): an error in the middle of level LSFM_TEST_FAIL_LEVEL (default 0);
// undone: a system reported above its bound at the end of the pass
struct Inject { int level = -1; bool undone = false; };
Inject test_switches(const lsfm_context* ctx, int attempt)
{
	Inject inj;
	if (!ctx->comm) return inj;
	static const char* frank = getenv("LSFM_TEST_FAIL_RANK");
	static int injected = 0; // (once per process: the run after the failed one must go through)
	if (frank && attempt == 0 && atoi(frank) == ctx->comm->rank && !injected++)
	{
		const char* kind = getenv("LSFM_TEST_FAIL_KIND");
		if (kind && !strcmp(kind, "undone")) inj.undone = true;
		else inj.level = getenv("LSFM_TEST_FAIL_LEVEL") ? atoi(getenv("LSFM_TEST_FAIL_LEVEL")) : 0;
	}
	return inj;
}

// One attempt: a pass over the tree, and what an Error thrown from it means for the run.
enum class Pass { DONE, AGAIN, AGAIN_GROWN };
Pass run_pass(lsfm_context* ctx, lsfm_tree* t, lsfm_stats* st, int attempt, int inject_level, std::unique_ptr<Error>& pass_error)
{
	try { tree_pass(ctx, t, st, inject_level); }
	catch (const Error& e)
	{
		if (ctx->comm)
		{
			// feature-sharded run: an error of this rank alone (LSFM_FAIL inside the pass) must still reach the exchange of the flags, or
			// its peers would wait there for a sum this rank never joins; it is rethrown after the exchange
			pass_error.reset(new Error(e));
			(void)hipStreamSynchronize(ctx->stream); (void)hipGetLastError();
			ctx->quiesce_side_streams();
			ctx->drop_prepared();
			return Pass::DONE;
		}
		// a level that was recording its plan found a pivot far below zero itself (lsfm_pcg.hip pcg_run): treated like the
		// same finding at the end of a run (run_verdict) -- the tree is joined again while attempts are left
		if (e.code == LSFM_ERR_NOT_SPD && attempt < 3)
		{
			(void)hipStreamSynchronize(ctx->stream); (void)hipGetLastError();
			ctx->quiesce_side_streams();
			ctx->stats = st; ctx->plan = nullptr; // (tree_pass was left mid-level)
			t->step_hint.clear(); t->plans.clear();
			if (getenv("LSFM_DEBUG_CONV")) fprintf(stderr, "[lsfm conv] attempt %d: %s -- joining the tree again\n", attempt, e.msg.c_str());
			return Pass::AGAIN;
		}
		ctx->quiesce_side_streams(); // (the pass was left mid-level: nothing of it may still be running when arenas grow or the caller resets them)
		// (the arenas start at an eighth of the upper bound the upload asked for: a run that exhausts one doubles them and starts over)
		if (e.code != LSFM_ERR_OOM || !ctx->grow_arenas()) throw;
		if (getenv("LSFM_DEBUG")) fprintf(stderr, "[lsfm] arenas grown to %zu MiB each after: %s\n", ctx->arena_bytes >> 20, e.msg.c_str());
		return Pass::AGAIN_GROWN; // (not a numerical repeat)
	}
	return Pass::DONE;
}

// LSFM_TIMELINE=1: where the enqueuing thread was when, in us since the mark before
void print_timeline(const lsfm_context* ctx)
{
	double prev = ctx->timeline.empty() ? 0 : ctx->timeline[0].second;
	for (const auto& m : ctx->timeline)
	{
		if (!strcmp(m.first, "level")) fprintf(stderr, "\n[tl]");
		fprintf(stderr, " %s+%.0f", m.first, 1e3 * (m.second - prev));
		prev = m.second;
	}
	fprintf(stderr, "\n");
}

// Feature-sharded run: whether the run is repeated (run_verdict) must be decided alike on every rank -- a rank that went on alone
// would wait for sums nobody else takes part in.  The ranks sum eight flags; rs / st come back as every rank's common view.
// pass_error: this rank's pass threw (rethrown here, once its peers know).
void exchange_flags(lsfm_context* ctx, lsfm_tree* t, RunStatsDev& rs, lsfm_stats* st, bool inject_undone, const Error* pass_error)
{
	Comm& cm = *ctx->comm;
	if (inject_undone) rs.undone++;
	if (pass_error)
	{
		// this rank left the pass alone, somewhere between two sums: it takes part in its peers' sums (with zeros) until they
		// are here too -- see Comm in lsfm_internal.hpp.  No healthy rank left, or the communicator itself failed: nothing to
		// exchange, the error is this rank's own
		bool there = false;
		try { there = cm.follow(ctx->stream); } catch (const Error&) { there = false; }
		if (!there) throw *pass_error;
	}
	cm.restart();
	long long* d_fl = cm.alloc<long long>(8);
	// (st->not_converged: what the levels that recorded a plan reported through the stats; fl[6]: this rank's pass threw)
	long long fl[8] = { rs.tr_err != 0, rs.chol_err != 0, rs.plan_stale != 0, rs.not_converged, rs.undone, st->not_converged, pass_error ? 1 : 0, 0 };
	LSFM_CHECK_HIP(hipMemcpyAsync(d_fl, fl, sizeof fl, hipMemcpyHostToDevice, ctx->stream));
	LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
	if (pass_error) cm.call(ctx->stream, (size_t)(reinterpret_cast<char*>(d_fl) - cm.buf), 8, LSFM_DTYPE_I64); // (its header went with follow())
	else cm.allreduce(ctx->stream, d_fl, 8, LSFM_DTYPE_I64, Comm::KIND_FINAL);
	LSFM_CHECK_HIP(hipMemcpyAsync(fl, d_fl, sizeof fl, hipMemcpyDeviceToHost, ctx->stream));
	LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
	if (fl[0] && !rs.tr_err) rs.tr_err = 1;
	if (fl[1] && !rs.chol_err) rs.chol_err = 1;
	rs.plan_stale = fl[2] != 0;
	rs.not_converged = (int)((fl[3] + cm.world - 1) / cm.world); // (every rank solves every system: the count, not its multiple)
	rs.undone = (int)((fl[4] + cm.world - 1) / cm.world);
	st->not_converged = (int)((fl[5] + cm.world - 1) / cm.world); // (the same verdict on every rank: run_verdict reads it)
	// (a failed pass may have left plans and step counts of levels it ran on zeros: the next run starts without them, alike
	// on every rank)
	if (pass_error || fl[6]) { t->plans.clear(); t->step_hint.clear(); }
	if (pass_error) throw *pass_error;
	if (fl[6]) LSFM_FAIL(LSFM_ERR_INTERNAL, "another rank of the feature-sharded run failed");
}

// What becomes of a pass that ran through, from its record, its stats and the attempts so far (host only; an Error: the run fails).
// Repeating a run.  A plan that met values it does not fit (LevelPlan::tr_sign), refinement steps enqueued by a count
// from an earlier run that did not suffice this time (`undone`), or a system left above its bound although every level
// asked after every step -- seen in one synth-16k Mono tree out of fifteen: the last 6x6 block of the root's top
// separator, what is left of 1e6..1e8-sized entries after 16 000 columns of updates whose atomic sums land in another
// order every run, came out slightly indefinite and its factor, taken by magnitude (k_sn_panel), was too poor a
// preconditioner.  In each case the tree is joined again without what the earlier runs left (plans, step counts): the
// rounding falls differently.  At most three times; what is still not converged then is reported (LSFM_NOT_CONVERGED).
enum class Verdict { ACCEPT, AGAIN_WITHOUT_PLANS, AGAIN_WITHOUT_PLANS_AND_HINTS };
Verdict run_verdict(const RunStatsDev& rs, const lsfm_stats& st, int attempt)
{
	const bool more = attempt < 3; // attempts left
	if (rs.tr_err) LSFM_FAIL(LSFM_ERR_ARG, "transform: target pose id not found in map " + std::to_string(rs.tr_err - 1));
	if (rs.chol_err && !more)
		LSFM_FAIL(LSFM_ERR_NOT_SPD, "Schur system is not positive definite (block column " + std::to_string(rs.chol_err - 1) + " of the factor)");
	if (rs.plan_stale)
	{
		if (!more) LSFM_FAIL(LSFM_ERR_INTERNAL, "level plans kept being reported stale");
		return Verdict::AGAIN_WITHOUT_PLANS;
	}
	// A pivot far below zero (k_sn_panel: more than 1 % of the diagonal entry S had) is reported as "not positive definite" --
	// after the other attempts: it was seen once in ~400 runs of the synth-16k Mono tree, at the last block of the root
	// (16 382 columns of updates above it), where a run before or after it factors a system that differs in the last bits
	// of S (K9's sums are floating-point atomics) without complaint.  A system that IS indefinite fails three times.
	// (st.not_converged: a level that records its plan reports through the stats, not the device record)
	if ((rs.chol_err || rs.not_converged || rs.undone || st.not_converged) && more) return Verdict::AGAIN_WITHOUT_PLANS_AND_HINTS;
	return Verdict::ACCEPT;
}

// the attempts of one run, until a pass is accepted (or an Error ends the run)
void run_attempts(lsfm_context* ctx, lsfm_tree* t, lsfm_stats* st)
{
	const double t_begin = now_ms();
	for (int attempt = 0;; attempt++)
	{
		memset(st, 0, sizeof *st);
		st->attempts = attempt + 1;
		ctx->timed.clear(); ctx->ev_next = 0;
		ctx->timeline_on = getenv("LSFM_TIMELINE") != nullptr;
		ctx->timeline.clear();
		ctx->mark("run");
		const Inject inj = test_switches(ctx, attempt);
		std::unique_ptr<Error> pass_error;
		const Pass pass = run_pass(ctx, t, st, attempt, inj.level, pass_error);
		if (pass == Pass::AGAIN_GROWN) attempt--;
		if (pass != Pass::DONE) continue;
		st->t_total_ms = now_ms() - t_begin; // (repeated attempts included; the stage times below are the last attempt's)
		ctx->mark("end");
		if (ctx->timeline_on) print_timeline(ctx);
		// what the warm levels left in the device accumulators instead of stopping for it
		RunStatsDev rs;
		LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream2)); // (the side stream's share of the record: k_sum_run_squares)
		LSFM_CHECK_HIP(hipMemcpy(&rs, ctx->d_run, sizeof rs, hipMemcpyDeviceToHost));
		if (ctx->comm) exchange_flags(ctx, t, rs, st, inj.undone, pass_error.get());
		if (rs.floored && getenv("LSFM_DEBUG_CONV")) fprintf(stderr, "[lsfm conv] %d pivot(s) of the separators held at their lower bound in this run\n", rs.floored);
		const Verdict v = run_verdict(rs, *st, attempt);
		if (v == Verdict::ACCEPT)
		{
			st->not_converged += rs.not_converged;
			st->max_rel_residual = std::max(st->max_rel_residual, rs.max_rel_residual);
			st->upload_ms = t->upload_ms;
			st->schur_flops += 108.0 * (double)rs.k2;
			st->s_digest = rs.s_digest; st->factor_digest = rs.factor_digest; st->refactor_mismatch = rs.refactor_mismatch; st->s_rebuild_mismatch = rs.s_rebuild_mismatch;
			return;
		}
		if (v == Verdict::AGAIN_WITHOUT_PLANS_AND_HINTS)
		{
			if (rs.chol_err && getenv("LSFM_DEBUG_CONV")) fprintf(stderr, "[lsfm conv] attempt %d: pivot of block column %d far below zero, joining the tree again\n", attempt, rs.chol_err - 1);
			t->step_hint.clear();
		}
		t->plans.clear();
	}
}

} // namespace

int tree_run(lsfm_context* ctx, lsfm_tree* t, lsfm_stats* stats)
{
	lsfm_stats local;
	memset(&local, 0, sizeof local);
	lsfm_stats* st = stats ? stats : &local;
	struct InRun {
		lsfm_context* c;
		InRun(lsfm_context* x, Comm* cm, lsfm_stats* s) : c(x) { c->in_tree_run = true; c->comm = cm; c->stats = s; }
		~InRun() { c->in_tree_run = false; c->comm = nullptr; c->stats = nullptr; }
	} in_run(ctx, t->comm.fn ? &t->comm : nullptr, st);
	LSFM_CHECK_HIP(hipStreamSynchronize(ctx->stream));
	run_attempts(ctx, t, st);
	ctx->flush_times();
	if (getenv("LSFM_LEVEL_GAPS")) { fprintf(stderr, "[lsfm] device idle between the levels of this run: %.3f ms\n", ctx->dbg_gap_ms); ctx->dbg_gap_ms = 0.0; }
	t->done = true;
	t->generation = ctx->generation;
	return st->not_converged ? LSFM_NOT_CONVERGED : LSFM_OK;
}

} // namespace lsfm
