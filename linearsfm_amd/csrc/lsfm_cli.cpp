// LinearSFM command line on top of liblsfm_hip: same flags, files and progress lines as the reference's console
// program (main: linux/src/LinearSFM/LinearSFM.cpp:9-18, parser: LinearSFMImp.cpp:7989-8087, help: 8089-8105).
//   LinearSFM -path <dir> -num <N> -type Monocular|Stereo [-p <poses>] [-f <features>] [-st <state>] [-help]
// Extra flags that do not collide with the reference's: -gpu <ordinal>, -tol <pcg rel tol>, -full <file> (final state
// at %.17g), -info <file> (final map WITH its information matrix in the local-map format), -stats 1 (timing breakdown
// on stderr: device stages of the join tree, then the wall seconds of every phase from files to files), -levels <L> -nodes <dir>
// (level checkpoint: stop after L tree levels and write the nodes of that level as <dir>/localmap_1.txt ...; a later run with
// -path <dir> -num <nodes> finishes the tree and gives the result of the uninterrupted run), -quiet 1 (no progress lines).
// -cache <file> (binary cache of the set: read instead of the text files when it holds -num maps of -type, written after the text files
// were parsed otherwise), -fullbin <file> (final state as raw doubles), -json <file> (the run's lsfm_stats and phase times as one JSON object),
// -gn <steps> (Gauss-Newton polish of the map-joining objective from the tree's result: lsfm_gn_polish; no reference counterpart),
// -cov <file> / -covf <file> (marginal covariances of the final map's poses / features: lsfm_map_covariance; no reference counterpart),
// -covcols <file> -covposes <id,id,...> (whole columns of the covariance for the poses with these labels: lsfm_map_covariance_columns; one
// line per (requested pose, pose): "id_q id_p" and the 36 entries of Sigma_{p,q}; the two flags go together),
// -gate <pairs file> -gateout <file> (the exact gate "are these two features one point": the pairs file holds whitespace-separated feature
// ids, two per candidate; one line per pair in input order, "id_f id_g d2" and the six upper entries of Sigma_d = Var(x_f - x_g) at %.17g:
// lsfm_map_feature_pair_gate; written after -covcols and before -chi2 through a temporary file renamed into place; the two flags go together;
// an unreadable file, an odd count, a pair naming one id twice or an id the final map does not have end the run non-zero with no file
// written; with -keepf / -keepp / -relin the ids are resolved in the map the other covariance files describe; no reference counterpart),
// -merge <pairs file> [-mergeout <file>] (declare the feature pairs of the file -- the -gate format, the same refusals -- one point each:
// after -gn / -relin and BEFORE -keepf / -keepp and before any file is written the final map is replaced by the merged map of
// lsfm_map_merge_features, so -st, -p, -f, -full, -fullbin, -info, -cov, -covf, -covcols and -gate describe the merged map, and a -gate id that
// was merged away is "no feature"; -mergeout: line 1 "K features_removed dof D2", then "id_f id_g id_kept" per pair at %.17g, written after
// -gateout through a temporary file renamed into place; not together with -chi2 / -chi2f -- the local maps still hold the merged-away ids --:
// that ends the run non-zero before any file is written; a numerical failure ends the run as -gate's does; no reference counterpart),
// -cand <file> -candr <radius> [-candtau <tau>] (the candidate pairs for -gate / -merge from the final map alone -- the map -gate resolves its
// ids in: after -gn, -relin, -merge, -keepf and -keepp: every pair of features within <radius> of each other and, with -candtau, whose bound
// q = 1/2 d^T (Sigma_ff + Sigma_gg)^-1 d is <= tau -- never above the gate's d2, so no pair the gate accepts at tau is lost:
// lsfm_map_feature_pair_candidates; with -candtau the feature covariances are lsfm_map_covariance's, computed once and shared with -cov / -covf;
// the file is a pair list of the features' ids in the call's order, the format -gate and -merge read, written after -mergeout and before
// -chi2 through a temporary file renamed into place; -cand without -candr, -candr or -candtau without -cand, a value that is not a positive
// number or a refusal of the library end the run non-zero before any file is written; feeding the file to -gate in the same run is not
// offered: -gate validates its file before anything is computed; no reference counterpart),
// -jgate <pairs file> -jgateout <file> [-jgatetau <tau>] [-jgatepairs <file>] (which of the candidate pairs are compatible TOGETHER: the sequential
// joint-compatibility selection of lsfm_map_feature_pair_joint_gate in ascending order of the individual d2, tau = chi^2_3 at 0.99 unless
// -jgatetau gives a positive number or inf; the pairs file is -gate's format with -gate's refusals and the ids are resolved in the map -gate
// resolves them in; -jgateout: line 1 "K accepted implied dof D2", then per pair in input order "id_f id_g status d2 delta" at %.17g, status 1
// accepted, 2 implied by the accepted pairs, 0 rejected; -jgatepairs: the accepted pairs as a pair list -- exactly what -merge reads in a later
// run; everything is computed before any file is written, the files follow -gateout and precede -mergeout, each through a temporary file
// renamed into place; -jgate without -jgateout or the reverse, -jgatetau / -jgatepairs without -jgate, more than 2048 pairs or a refusal of the
// library end the run non-zero with nothing written; no reference counterpart),
// -robust huber|cauchy <c> (-gn uses lsfm_gn_polish_robust: whole local maps down-weighted by an M-estimator on chi2_k / dof_k),
// -chi2 <file> (per local map, in input order, "index dof chi2 weight" at the final state: lsfm_map_chi2; no reference counterpart),
// -robustf huber|cauchy <c> (-gn uses lsfm_gn_polish_robust_features: single features of single local maps down-weighted by an M-estimator on
// their conditional chi2 c_kf / 3; not together with -robust or -relin: the two estimators are not combined, and the linearisation with
// the feature weights is a flag of its own, -relinf),
// -chi2f <file> (per local map and feature, in input order, "map_index feature_id chi2 weight" at the final state: lsfm_map_feature_chi2, the
// weight 1 without -robustf; written after -chi2 through a temporary file renamed into place; no reference counterpart),
// -relin 1 (the final map's information matrix -- U / W / V and their index arrays -- is replaced by the local maps linearised at the final
// state, after -gn if given and with the polish's weights under -robust: lsfm_gn_linearise; -info, -cov, -covf and -covcols then describe
// the estimate the other files hold; no reference counterpart),
// -relinf 1 (with -gn and -robustf, at the place -relin acts: the final map's U / W / V and their index arrays are replaced by the local
// maps linearised at the polished state WITH the polish's feature weights, lsfm_gn_linearise_features -- the matrix the last feature-robust
// step solved with; every later flag then describes that map; -st, -p, -f and -chi2f are what they are without it; without -robustf,
// together with -relin or on a library error the run ends non-zero before any file is written; no reference counterpart),
// -keepf <file> (whitespace-separated feature ids, unknown ones ignored: after -gn / -relin and before any file is written the final map is
// replaced by its reduction to these features -- every other feature marginalised out, lsfm_map_marginalise; -st, -p, -f, -full, -fullbin,
// -info, -cov, -covf and -covcols describe the reduced map, -chi2 is evaluated on the full state first; no reference counterpart),
// -keepp <file> (whitespace-separated pose ids, unknown ones ignored: at the same place the final map is replaced by its reduction to these
// poses -- every other pose marginalised out together with the features it sees, lsfm_map_marginalise_poses: a key-frame map.  With -keepf
// the dropped features are those -keepf drops plus those a dropped pose sees.  The files describe the reduced map as under -keepf; -covposes
// naming a dropped pose, an unreadable file or a list without the gauge poses (Ref; Monocular: ScaP too) end the run non-zero with no file
// written; no reference counterpart).
#include <cmath>
#include <chrono>
#include <sys/stat.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/lsfm.h"

static void print_help()
{
	printf("Linear SFM Solution General Options\n");
	printf("\n");
	printf("-path			Set Data Path.\n");
	printf("-st            Set Path to Save Final State Vector\n");
	printf("-p			Set Path to Save Poses\n");
	printf("-f			Set Path to Save Features\n");
	printf("-num			Number of Initial Recontruction\n");
	printf("-type			Set Data Type.\n");
	printf("Data Type Listed As Following:\n");
	printf("			I  : Monocular\n");
	printf("			II : Stereo\n");
	printf("-robust huber|cauchy <c>	With -gn: Down-Weight Inconsistent Local Maps (Threshold c On chi2 / dof)\n");
	printf("-chi2 <file>		Save chi2 Of Every Local Map: index dof chi2 weight\n");
	printf("-robustf huber|cauchy <c>	With -gn: Down-Weight Inconsistent Single Features (Threshold c On Their chi2 / 3); Not With -robust Or -relin (See -relinf)\n");
	printf("-chi2f <file>		Save chi2 Of Every Feature Of Every Local Map: map_index feature_id chi2 weight\n");
	printf("-relin 1		Information Matrix (-info, -cov, -covf, -covcols) Of The Local Maps Linearised At The Final State\n");
	printf("-relinf 1		With -gn And -robustf: The Same With The Polish's Feature Weights (The Matrix Of Its Last Step); Not With -relin\n");
	printf("-keepf <file>		Keep Only The Features Whose Ids The File Lists: The Others Are Marginalised Out Of The Final Map\n");
	printf("-gate <file> -gateout <file>	Gate Candidate Feature Pairs (Two Ids Each): id_f id_g d2 And The Upper Triangle Of Var(x_f - x_g)\n");
	printf("-merge <file> [-mergeout <file>]	Merge Feature Pairs (Two Ids Each) Into One Point Each; Report: K removed dof D2, Then id_f id_g id_kept\n");
	printf("-cand <file> -candr <radius> [-candtau <tau>]	Save The Candidate Feature Pairs For -gate / -merge: Within <radius>, And With -candtau Bound q <= tau\n");
	printf("-jgate <file> -jgateout <file> [-jgatetau <tau>] [-jgatepairs <file>]	Select The Jointly Compatible Feature Pairs: K accepted implied dof D2, Then id_f id_g status d2 delta\n");
	printf("-keepp <file>		Keep Only The Poses Whose Ids The File Lists: The Others Are Marginalised Out Of The Final Map\n");
	printf("\n");
}

int main(int argc, char** argv)
{
	std::string path, st, pose, fea, full, info, nodes, cache, fullbin, json, cov, covf, chi2f, robust_err, covcols, covposes, keepf, keepp, chi2ff, gate, gateout, merge, mergeout, cand, candr, candtau, jgate, jgateout, jgatetau, jgatepairs;
	int num = 0, type = -1, gpu = 0, want_stats = 0, levels = 0, quiet = 0, gn = 0, robust = 0, relin = 0, robustf = 0, relinf = 0;
	double robust_c = 0.0, robustf_c = 0.0;
	bool has_path = false, has_num = false, has_keepf = false, has_keepp = false, has_gate = false, has_gateout = false, has_merge = false, has_mergeout = false, has_cand = false, has_candr = false, has_candtau = false;
	bool has_jgate = false, has_jgateout = false, has_jgatetau = false, has_jgatepairs = false;
	double tol = 0;
	for (int i = 1; i < argc; i++)
	{
		std::string name = argv[i];
		if (name[0] != '-') return 0; // each param has to start with at least one dash (Imp.cpp:8000-8002)
		size_t d = name.find_first_not_of('-');
		if (d != std::string::npos) name = name.substr(d);
		if (name == "help") { print_help(); return 0; }
		auto next = [&]() -> const char* { return (i + 1 < argc) ? argv[++i] : ""; };
		if (name == "path") { path = next(); has_path = true; }
		else if (name == "st") st = next();
		else if (name == "p") pose = next();
		else if (name == "f") fea = next();
		else if (name == "num") { num = atoi(next()); has_num = true; }
		else if (name == "type")
		{
			std::string v = next();
			if (v == "Monocular") type = 1;
			if (v == "Stereo") type = 0;
		}
		else if (name == "gpu") gpu = atoi(next());
		else if (name == "tol") tol = atof(next());
		else if (name == "full") full = next();
		else if (name == "info") info = next();
		else if (name == "stats") want_stats = atoi(next());
		else if (name == "levels") levels = atoi(next());
		else if (name == "nodes") nodes = next();
		else if (name == "quiet") quiet = atoi(next());
		else if (name == "cache") cache = next();
		else if (name == "fullbin") fullbin = next();
		else if (name == "json") json = next();
		else if (name == "gn") gn = atoi(next());
		else if (name == "cov") cov = next();
		else if (name == "covf") covf = next();
		else if (name == "chi2") chi2f = next();
		else if (name == "relin") relin = atoi(next());
		else if (name == "relinf") relinf = atoi(next());
		else if (name == "covcols") covcols = next();
		else if (name == "covposes") covposes = next();
		else if (name == "keepf") { keepf = next(); has_keepf = true; }
		else if (name == "keepp") { keepp = next(); has_keepp = true; }
		else if (name == "chi2f") chi2ff = next();
		else if (name == "gate") { gate = next(); has_gate = true; }
		else if (name == "gateout") { gateout = next(); has_gateout = true; }
		else if (name == "merge") { merge = next(); has_merge = true; }
		else if (name == "mergeout") { mergeout = next(); has_mergeout = true; }
		else if (name == "cand") { cand = next(); has_cand = true; }
		else if (name == "candr") { candr = next(); has_candr = true; }
		else if (name == "candtau") { candtau = next(); has_candtau = true; }
		else if (name == "jgate") { jgate = next(); has_jgate = true; }
		else if (name == "jgateout") { jgateout = next(); has_jgateout = true; }
		else if (name == "jgatetau") { jgatetau = next(); has_jgatetau = true; }
		else if (name == "jgatepairs") { jgatepairs = next(); has_jgatepairs = true; }
		else if (name == "robust" || name == "robustf")
		{
			const std::string k = next(), v = next();
			char* end = nullptr;
			const double c = strtod(v.c_str(), &end);
			const int kind = k == "huber" ? 1 : (k == "cauchy" ? 2 : 0);
			if (name == "robust") { robust = kind; robust_c = c; } else { robustf = kind; robustf_c = c; }
			if (!kind) robust_err = "-" + name + ": the kind must be huber or cauchy (got '" + k + "')";
			else if (v.empty() || *end || !std::isfinite(c) || c <= 0) robust_err = "-" + name + " " + k + " <c>: c must be a positive number (got '" + v + "')";
		}
	}
	if (!has_path) { printf("LinerSFM Error: Please Input Right File Path:\n"); return 0; }
	if (!has_num) { printf("LinerSFM Error: Please Set Local Map Number:\n"); return 0; }
	if (type < 0) { printf("LinerSFM Error: Please Set Data Type:\n"); return 0; }
	if (num <= 0) { fprintf(stderr, "LinearSFM: -num must be positive (got %d)\n", num); return 1; }
	if ((levels > 0) != !nodes.empty() || levels < 0) { fprintf(stderr, "LinearSFM: -levels <L > 0> and -nodes <dir> go together\n"); return 1; }
	if (!robust_err.empty()) { fprintf(stderr, "LinearSFM: %s\n", robust_err.c_str()); return 1; }
	if (covcols.empty() != covposes.empty()) { fprintf(stderr, "LinearSFM: -covcols <file> and -covposes <id,id,...> go together\n"); return 1; }
	std::vector<int> covids;
	for (size_t p = 0; p < covposes.size();)
	{
		char* end = nullptr;
		const long v = strtol(covposes.c_str() + p, &end, 10);
		if (end == covposes.c_str() + p || (*end && *end != ',') || (*end == ',' && !end[1])) { fprintf(stderr, "LinearSFM: -covposes: '%s' is not a list of pose ids\n", covposes.c_str()); return 1; }
		covids.push_back((int)v);
		p = (size_t)(end - covposes.c_str()) + (*end ? 1 : 0);
	}
	// -keepf / -keepp: the ids to keep, sorted; an unreadable file ends the run before anything is computed or written
	std::vector<int> keepids, keeppids;
	auto read_ids = [](const char* flag, const char* what, const std::string& fn, std::vector<int>& ids) {
		FILE* f = fopen(fn.c_str(), "r");
		if (!f) { fprintf(stderr, "LinearSFM: %s: cannot read %s\n", flag, fn.c_str()); return false; }
		int v = 0, got = 0;
		while ((got = fscanf(f, "%d", &v)) == 1) ids.push_back(v);
		const bool junk = got != EOF;
		fclose(f);
		if (junk) { fprintf(stderr, "LinearSFM: %s: %s is not a list of %s ids\n", flag, fn.c_str(), what); return false; }
		std::sort(ids.begin(), ids.end());
		return true;
	};
	if (has_keepf && !read_ids("-keepf", "feature", keepf, keepids)) return 1;
	if (has_keepp && !read_ids("-keepp", "pose", keepp, keeppids)) return 1;
	// -gate: the candidate pairs by label, in input order; a file that cannot be a list of pairs ends the run before anything is computed
	std::vector<int> gateids, mergeids;
	auto read_pairs = [](const char* flag, const std::string& fn, std::vector<int>& ids) {
		FILE* f = fopen(fn.c_str(), "r");
		if (!f) { fprintf(stderr, "LinearSFM: %s: cannot read %s\n", flag, fn.c_str()); return false; }
		int v = 0, got = 0;
		while ((got = fscanf(f, "%d", &v)) == 1) ids.push_back(v);
		fclose(f);
		if (got != EOF || ids.empty() || ids.size() % 2) { fprintf(stderr, "LinearSFM: %s: %s is not a list of feature id pairs\n", flag, fn.c_str()); return false; }
		for (size_t a = 0; a < ids.size(); a += 2)
			if (ids[a] == ids[a + 1]) { fprintf(stderr, "LinearSFM: %s: a pair names feature %d twice\n", flag, ids[a]); return false; }
		return true;
	};
	if (has_gate != has_gateout || (has_gate && (gate.empty() || gateout.empty()))) { fprintf(stderr, "LinearSFM: -gate <pairs file> and -gateout <file> go together\n"); return 1; }
	if (has_gate && !read_pairs("-gate", gate, gateids)) return 1;
	// -merge: the pairs to merge, the same format and refusals
	if ((has_mergeout && !has_merge) || (has_merge && merge.empty()) || (has_mergeout && mergeout.empty())) { fprintf(stderr, "LinearSFM: -mergeout <file> needs -merge <pairs file>\n"); return 1; }
	if (has_merge && (!chi2f.empty() || !chi2ff.empty()))
	{
		fprintf(stderr, "LinearSFM: -merge does not go together with -chi2 / -chi2f: the local maps still hold the merged-away ids\n");
		return 1;
	}
	if (has_merge && !read_pairs("-merge", merge, mergeids)) return 1;
	// -cand: the flags go together and their values are positive numbers, before anything is computed
	double cand_radius = 0.0, cand_tau = 0.0;
	if (has_cand && (!has_candr || cand.empty())) { fprintf(stderr, "LinearSFM: -cand <file> needs -candr <radius>\n"); return 1; }
	if ((has_candr || has_candtau) && !has_cand) { fprintf(stderr, "LinearSFM: -candr <radius> and -candtau <tau> need -cand <file>\n"); return 1; }
	auto positive = [](const char* flag, const std::string& v, double& x) {
		char* end = nullptr;
		x = strtod(v.c_str(), &end);
		if (v.empty() || *end || !std::isfinite(x) || x <= 0) { fprintf(stderr, "LinearSFM: %s: '%s' is not a positive number\n", flag, v.c_str()); return false; }
		return true;
	};
	if (has_candr && !positive("-candr", candr, cand_radius)) return 1;
	if (has_candtau && !positive("-candtau", candtau, cand_tau)) return 1;
	// -jgate: the flags go together, the file is a list of pairs and tau a positive number (inf allowed), before anything is computed
	std::vector<int> jgateids;
	double jgate_tau = 11.344866730144373; // chi^2_3 at 0.99
	if (has_jgate != has_jgateout || (has_jgate && (jgate.empty() || jgateout.empty()))) { fprintf(stderr, "LinearSFM: -jgate <pairs file> and -jgateout <file> go together\n"); return 1; }
	if ((has_jgatetau || has_jgatepairs) && !has_jgate) { fprintf(stderr, "LinearSFM: -jgatetau <tau> and -jgatepairs <file> need -jgate <pairs file>\n"); return 1; }
	if (has_jgatepairs && jgatepairs.empty()) { fprintf(stderr, "LinearSFM: -jgatepairs needs a file name\n"); return 1; }
	if (has_jgatetau)
	{
		char* end = nullptr;
		jgate_tau = strtod(jgatetau.c_str(), &end);
		if (jgatetau.empty() || *end || !(jgate_tau > 0)) { fprintf(stderr, "LinearSFM: -jgatetau: '%s' is not a positive number\n", jgatetau.c_str()); return 1; }
	}
	if (has_jgate && !read_pairs("-jgate", jgate, jgateids)) return 1;
	if (jgateids.size() / 2 > LSFM_JOINT_GATE_MAX) { fprintf(stderr, "LinearSFM: -jgate: %zu pairs, at most %d\n", jgateids.size() / 2, LSFM_JOINT_GATE_MAX); return 1; }
	if (robust && gn <= 0) { fprintf(stderr, "LinearSFM: -robust applies to -gn <steps>: give -gn too\n"); return 1; }
	if (robustf && gn <= 0) { fprintf(stderr, "LinearSFM: -robustf applies to -gn <steps>: give -gn too\n"); return 1; }
	if (robustf && robust) { fprintf(stderr, "LinearSFM: -robustf and -robust do not go together: the map and the feature estimator are not combined\n"); return 1; }
	if (robustf && relin) { fprintf(stderr, "LinearSFM: -robustf and -relin do not go together: linearising with feature weights is not offered\n"); return 1; }
	if (relinf && relin) { fprintf(stderr, "LinearSFM: -relinf and -relin do not go together: the final map is one linearisation or the other\n"); return 1; }
	if (relinf && !robustf) { fprintf(stderr, "LinearSFM: -relinf applies to -gn <steps> -robustf <kind> <c>: it linearises with that polish's feature weights\n"); return 1; }

	auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
	const double w0 = now();
	std::vector<lsfm_map> maps(num);
	bool from_cache = false;
	// what a cache must have been made from to be believed: the resolved directory and size + modification time of its first n text files
	// (FNV-1a; 0 is "no stamp": never produced)
	auto source_stamp = [&](int n, bool* all_there) {
		unsigned long long h = 1469598103934665603ull;
		auto mix = [&](const void* p, size_t len) { const unsigned char* b = static_cast<const unsigned char*>(p); for (size_t i = 0; i < len; i++) { h ^= b[i]; h *= 1099511628211ull; } };
		char* rp = realpath(path.c_str(), nullptr);
		const std::string dir = rp ? rp : path;
		free(rp);
		mix(dir.data(), dir.size());
		*all_there = true;
		for (int k = 1; k <= n; k++)
		{
			struct stat st;
			const std::string fn = path + "/localmap_" + std::to_string(k) + ".txt";
			if (stat(fn.c_str(), &st) != 0) { *all_there = false; return 0ull; }
			const long long v[3] = { (long long)st.st_size, (long long)st.st_mtim.tv_sec, (long long)st.st_mtim.tv_nsec };
			mix(v, sizeof v);
		}
		return h ? h : 1ull;
	};
	if (!cache.empty())
	{
		// the binary cache of an earlier run over this set: used when it holds what is asked for AND was made from the text files as they
		// are now (its stamp); (re)written otherwise.  Text files that are gone cannot contradict it: the cache is then all there is.
		int cn = 0, cm = 0;
		if (lsfm_mapset_info(cache.c_str(), &cn, &cm) == LSFM_OK && cn >= num && cm == type)
		{
			unsigned long long have = 0;
			bool there = false;
			const unsigned long long want = source_stamp(cn, &there);
			(void)lsfm_mapset_stamp(cache.c_str(), &have, nullptr);
			if (there && have != want)
				fprintf(stderr, "LinearSFM: %s was not made from the text files under %s as they are now: reading them again\n", cache.c_str(), path.c_str());
			else from_cache = lsfm_read_mapset(cache.c_str(), type, 0, num, 0, maps.data()) == LSFM_OK;
		}
		else if (cn) fprintf(stderr, "LinearSFM: %s does not hold %d %s maps: reading the text files\n", cache.c_str(), num, type ? "Monocular" : "Stereo");
	}
	if (!from_cache)
	{
		// localmap_1.txt ... localmap_<num>.txt (Imp.cpp:125), parsed on all host cores
		int bad = 0;
		if (lsfm_read_localmaps(path.c_str(), 1, num, type, 0, maps.data(), &bad))
		{
			fprintf(stderr, "LinearSFM: cannot read %s/localmap_%d.txt\n", path.c_str(), bad);
			return 1;
		}
		if (!cache.empty())
		{
			bool there = false;
			const unsigned long long stamp = source_stamp(num, &there);
			if (lsfm_write_mapset(cache.c_str(), maps.data(), num, type) || lsfm_mapset_stamp(cache.c_str(), nullptr, &stamp))
				fprintf(stderr, "LinearSFM: cannot write %s\n", cache.c_str());
		}
	}
	const double w1 = now();
	lsfm_context* ctx = nullptr;
	int rc = lsfm_context_create(gpu, 0, &ctx);
	if (rc) { fprintf(stderr, "LinearSFM: no HIP device (rc=%d); this build has no CPU path\n", rc); return 2; }
	if (tol > 0) lsfm_set_pcg(ctx, tol, 0);
	// progress lines of the reference (Imp.cpp:1952, 1995)
	if (!quiet)
	{
		int cnt = num, L = 0;
		while (cnt > 1 && (levels <= 0 || L < levels))
		{
			int N2 = cnt % 2;
			cnt = (int)(cnt / 2.0 + 0.5);
			for (int i = 0; i < cnt; i++)
			{
				int NumLM = (i < cnt - 1 || N2 == 0) ? 2 : 1;
				for (int j = 0; j < NumLM; j++) printf("Join Level %d Local Map %d\n", L, 2 * i + j + 1);
				printf("Generate Level %d Local Map %d\n\n", L + 1, i + 1);
			}
			L++;
		}
	}
	// what lsfm_divide_conquer does, in its three steps so that each can be timed: maps to the device, the join tree (the
	// region the reference times), the final map back
	lsfm_map out;
	lsfm_stats stats;
	lsfm_tree* tree = nullptr;
	const double w2 = now();
	rc = lsfm_tree_upload(ctx, maps.data(), num, type, &tree);
	if (rc < 0) { fprintf(stderr, "LinearSFM: %s\n", lsfm_last_error(ctx)); return 3; }
	lsfm_tree_set_plans(tree, 0); // one run: nothing to keep for a next one
	if (levels > 0) lsfm_tree_set_stop_level(tree, levels);
	const double w3 = now();
	rc = lsfm_tree_run(ctx, tree, &stats);
	if (rc < 0) { fprintf(stderr, "LinearSFM: %s\n", lsfm_last_error(ctx)); return 3; }
	const double w4 = now();
	const int nnodes = lsfm_tree_node_count(ctx, tree);
	if (levels > 0 && nnodes > 1)
	{
		// level checkpoint: the nodes of the level the run ended at, named like a set of local maps
		for (int k = 0; k < nnodes; k++)
		{
			lsfm_map node;
			if (lsfm_tree_download_node(ctx, tree, k, &node) < 0) { fprintf(stderr, "LinearSFM: %s\n", lsfm_last_error(ctx)); return 3; }
			const std::string fn = nodes + "/localmap_" + std::to_string(k + 1) + ".txt";
			const int wrc = lsfm_write_localmap(fn.c_str(), type, &node);
			lsfm_map_release(&node);
			if (wrc) { fprintf(stderr, "LinearSFM: cannot write %s\n", fn.c_str()); return 1; }
		}
		printf("Stopped After Level %d: %d Nodes Written To %s\n", levels, nnodes, nodes.c_str());
		printf("Total Used Time:  %lf  sec\n\n", stats.t_total_ms * 1e-3);
		lsfm_tree_free(ctx, tree);
		for (auto& g : maps) lsfm_map_release(&g);
		lsfm_context_destroy(ctx);
		return rc == LSFM_NOT_CONVERGED ? 4 : 0;
	}
	{
		const int drc = lsfm_tree_download(ctx, tree, &out);
		if (drc < 0) { fprintf(stderr, "LinearSFM: %s\n", lsfm_last_error(ctx)); return 3; }
	}
	lsfm_tree_free(ctx, tree);
	const double w5 = now();
	// the reference solves directly and cannot end half-way; a system the refinement left above its residual bound is
	// reported and reflected in the exit code (the files are still written)
	const bool partial = rc == LSFM_NOT_CONVERGED;
	if (partial)
		fprintf(stderr, "LinearSFM: WARNING: %d camera system(s) not solved to the residual of a direct solve (max relative residual %.3e)\n",
		        stats.not_converged, stats.max_rel_residual);
	printf("Total Used Time:  %lf  sec\n\n", stats.t_total_ms * 1e-3); // Imp.cpp:2072
	std::vector<double> chi2v, weightv; // -robust: per-map chi2 and weights at the polished state
	std::vector<double> fchi2v, fweightv; // -robustf: per-feature chi2 and weights at the polished state (every feature of every map, input order)
	size_t nfeat = 0;
	for (const lsfm_map& g : maps) nfeat += (size_t)g.n;
	if (gn > 0)
	{
		// -gn <steps>: Gauss-Newton polish of the map-joining objective over all local maps, from the tree's result (lsfm_gn_polish; the
		// reference has no such step -- without the flag the program is the reference's)
		std::vector<double> obj(gn + 1), gnorm(gn + 1);
		std::vector<int> halv(gn);
		const double g0 = now();
		if (robust) { chi2v.resize(num); weightv.resize(num); }
		if (robustf) { fchi2v.resize(nfeat + 1); fweightv.resize(nfeat + 1); }
		const int grc = robustf ? lsfm_gn_polish_robust_features(ctx, maps.data(), num, type, &out, gn, robustf, robustf_c, obj.data(), gnorm.data(), halv.data(), fchi2v.data(), fweightv.data())
		              : robust ? lsfm_gn_polish_robust(ctx, maps.data(), num, type, &out, gn, robust, robust_c, obj.data(), gnorm.data(), halv.data(), chi2v.data(), weightv.data())
		                       : lsfm_gn_polish(ctx, maps.data(), num, type, &out, gn, obj.data(), gnorm.data(), halv.data());
		if (grc < 0) { fprintf(stderr, "LinearSFM: %s\n", lsfm_last_error(ctx)); return 3; }
		if (!quiet)
		{
			for (int i = 0; i <= gn; i++) printf("Gauss-Newton Step %d: Objective %.9e  Gradient %.3e\n", i, obj[i], gnorm[i]);
			printf("Gauss-Newton Used Time:  %lf  sec\n\n", now() - g0);
		}
	}
	if (relin || relinf)
	{
		// -relin 1: the information matrix of the state the files hold -- the local maps linearised at it (under -robust with the weights the
		// polish ended at) instead of the tree's, whose joins linearised at states the estimate has since left.  -relinf 1: the same with
		// the feature weights -robustf ended at
		lsfm_map H;
		const int lrc = relinf ? lsfm_gn_linearise_features(ctx, maps.data(), num, type, &out, nullptr, fweightv.data(), &H, nullptr, nullptr)
		                       : lsfm_gn_linearise(ctx, maps.data(), num, type, &out, weightv.empty() ? nullptr : weightv.data(), &H, nullptr, nullptr);
		if (lrc != LSFM_OK)
		{
			fprintf(stderr, "LinearSFM: %s: %s\n", relinf ? "relinf" : "relin", lsfm_last_error(ctx));
			return 3;
		}
		lsfm_map_release(&out);
		out = H;
	}
	std::vector<int> mergekept; // -merge: per pair the label of the feature both became
	int merge_removed = 0, merge_dof = 0;
	double merge_d2 = 0.0;
	if (has_merge)
	{
		// the final map with the pairs of -merge declared one point each (lsfm_map_merge_features): what follows describes the merged map
		std::vector<int> mp;
		for (int id : mergeids)
		{
			int at = -1;
			for (int f = 0; f < out.n; f++) if (out.stno[6 * out.m + 3 * f] == id) at = f; // (the last state entry of an id, as the feature file)
			if (at < 0) { fprintf(stderr, "LinearSFM: -merge: the final map has no feature %d\n", id); return 3; }
			mp.push_back(at);
		}
		const int K = (int)mp.size() / 2;
		std::vector<int> rep(out.n > 0 ? out.n : 1);
		lsfm_map M;
		int steps = 0;
		const int mrc = lsfm_map_merge_features(ctx, &out, type, mp.data(), K, &M, &merge_d2, &merge_dof, rep.data(), &steps, nullptr);
		if (mrc < 0 || (mrc > 0 && steps == 0))
		{
			fprintf(stderr, "LinearSFM: merge: %s\n", mrc < 0 ? lsfm_last_error(ctx) : "pivots had to be floored (the merged information matrix is too close to singular)");
			return 3;
		}
		if (mrc > 0) fprintf(stderr, "LinearSFM: merge: the refinement took all %d steps and its last correction is still above the tolerance\n", steps);
		merge_removed = out.n - M.n;
		for (int a = 0; a < K; a++) mergekept.push_back(M.stno[6 * M.m + 3 * rep[mp[2 * a]]]);
		if (!quiet) printf("Merged %d Feature Pairs: %d Features Removed, D2 %.9e With %d Degrees Of Freedom\n\n", K, merge_removed, merge_d2, merge_dof);
		lsfm_map_release(&out);
		out = M;
	}
	std::vector<int> chi2dof; // -keepf with -chi2: filled before the reduction
	if (has_keepf || has_keepp)
	{
		// -chi2 needs the full state: evaluated now, its file is still written last
		if (!chi2f.empty() && chi2v.empty())
		{
			chi2v.resize(num); weightv.assign(num, 1.0); chi2dof.resize(num);
			if (lsfm_map_chi2(ctx, maps.data(), num, type, &out, chi2v.data(), chi2dof.data()) < 0) { fprintf(stderr, "LinearSFM: chi2: %s\n", lsfm_last_error(ctx)); return 3; }
		}
		if (!chi2ff.empty() && fchi2v.empty())
		{
			fchi2v.resize(nfeat + 1); fweightv.assign(nfeat + 1, 1.0);
			if (lsfm_map_feature_chi2(ctx, maps.data(), num, type, &out, fchi2v.data(), nullptr) < 0) { fprintf(stderr, "LinearSFM: chi2f: %s\n", lsfm_last_error(ctx)); return 3; }
		}
		// the final map reduced to the features of -keepf: every other one marginalised out (lsfm_map_marginalise); to the poses of -keepp:
		// every other one marginalised out, with the features it sees (lsfm_map_marginalise_poses)
		std::vector<unsigned char> drop(out.n > 0 ? out.n : 1, 0), keepflag(out.m, 1);
		if (has_keepf)
			for (int f = 0; f < out.n; f++) drop[f] = std::binary_search(keepids.begin(), keepids.end(), out.stno[6 * out.m + 3 * f]) ? 0 : 1;
		lsfm_map R;
		if (has_keepp)
		{
			for (int p = 0; p < out.m; p++) keepflag[p] = std::binary_search(keeppids.begin(), keeppids.end(), -out.stno[6 * p]) ? 1 : 0;
			for (int w = 0; w < out.nW; w++)
				if (!keepflag[out.photo[w]]) drop[out.feature[w]] = 1;
			const int prc = lsfm_map_marginalise_poses(ctx, &out, type, keepflag.data(), drop.data(), &R);
			if (prc != LSFM_OK)
			{
				fprintf(stderr, "LinearSFM: keepp: %s\n", prc < 0 ? lsfm_last_error(ctx) : "pivots had to be floored (the dropped poses' own system is too close to singular)");
				return 3;
			}
		}
		else if (lsfm_map_marginalise(ctx, &out, drop.data(), &R) != LSFM_OK)
		{
			fprintf(stderr, "LinearSFM: keepf: %s\n", lsfm_last_error(ctx));
			return 3;
		}
		lsfm_map_release(&out);
		out = R;
	}
	if (want_stats)
		fprintf(stderr, "lsfm: total %.3f ms (transform %.3f, join %.3f [schur %.3f, pcg %.3f, backsub %.3f]), pcg its %ld, max rel resid %.2e, not converged %d, attempts %d\n",
		        stats.t_total_ms, stats.t_transform_ms, stats.t_join_ms, stats.t_schur_ms, stats.t_pcg_ms, stats.t_backsub_ms, stats.pcg_iterations,
		        stats.max_rel_residual, stats.not_converged, stats.attempts);
	// -covposes: labels to poses of the final map, before any file is written (an unknown id: nothing is written)
	std::vector<int> q;
	for (int id : covids)
	{
		int at = -1;
		for (int p = 0; p < out.m; p++) if (-out.stno[6 * p] == id) at = p; // (the last state entry of an id, as the pose file)
		if (at < 0) { fprintf(stderr, "LinearSFM: -covposes: the final map has no pose %d\n", id); return 3; }
		for (int e : q) if (e == at) { fprintf(stderr, "LinearSFM: -covposes: pose %d is named twice\n", id); return 3; }
		q.push_back(at);
	}
	// -gate: labels to features of the final map, likewise
	std::vector<int> gatepairs;
	for (int id : gateids)
	{
		int at = -1;
		for (int f = 0; f < out.n; f++) if (out.stno[6 * out.m + 3 * f] == id) at = f; // (the last state entry of an id, as the feature file)
		if (at < 0) { fprintf(stderr, "LinearSFM: -gate: the final map has no feature %d\n", id); return 3; }
		gatepairs.push_back(at);
	}
	std::vector<int> jgatefeat;
	for (int id : jgateids)
	{
		int at = -1;
		for (int f = 0; f < out.n; f++) if (out.stno[6 * out.m + 3 * f] == id) at = f;
		if (at < 0) { fprintf(stderr, "LinearSFM: -jgate: the final map has no feature %d\n", id); return 3; }
		jgatefeat.push_back(at);
	}
	// marginal covariances of the final map (after -gn its information matrix is still the tree's, unless -relin 1): once, for -cov / -covf
	// and for -candtau
	std::vector<double> pc, fc;
	auto covariances = [&]() {
		if (!pc.empty()) return true;
		pc.resize((size_t)out.m * 36 + 1); fc.resize((size_t)out.n * 9 + 1);
		const int crc = lsfm_map_covariance(ctx, &out, type, pc.data(), fc.data(), nullptr, 0, nullptr);
		if (crc != LSFM_OK)
			fprintf(stderr, "LinearSFM: covariance: %s\n", crc < 0 ? lsfm_last_error(ctx) : "pivots had to be floored (the information matrix is too close to singular)");
		return crc == LSFM_OK;
	};
	// -cand: the candidate pairs of the final map, before any file is written (a refusal: nothing is written)
	std::vector<int> candids;
	long long ncand = 0;
	if (has_cand)
	{
		if (has_candtau && !covariances()) return 3;
		const double* sig = has_candtau ? fc.data() : nullptr;
		int crc = lsfm_map_feature_pair_candidates(ctx, &out, sig, cand_radius, cand_tau, nullptr, nullptr, nullptr, 0, &ncand);
		if (crc == LSFM_OK && ncand > 0)
		{
			candids.resize(2 * (size_t)ncand);
			crc = lsfm_map_feature_pair_candidates(ctx, &out, sig, cand_radius, cand_tau, candids.data(), nullptr, nullptr, ncand, &ncand);
		}
		if (crc != LSFM_OK) { fprintf(stderr, "LinearSFM: -cand: %s\n", lsfm_last_error(ctx)); return 3; }
		for (int& f : candids) f = out.stno[6 * out.m + 3 * f]; // indices to labels
	}
	// -jgate: the selection among the candidate pairs, before any file is written (a refusal or a numerical failure: nothing is written)
	std::vector<int> jstatus;
	std::vector<double> jdelta, jd2;
	int jacc = 0, jimp = 0;
	double jD2 = 0.0;
	if (has_jgate)
	{
		const int K = (int)jgatefeat.size() / 2;
		jstatus.resize(K); jdelta.resize(K); jd2.resize(K);
		int steps = 0;
		const int jrc = lsfm_map_feature_pair_joint_gate(ctx, &out, type, jgatefeat.data(), K, nullptr, jgate_tau, jstatus.data(), jdelta.data(), jd2.data(), nullptr,
		                                                 &jacc, &jimp, &jD2, &steps, nullptr);
		if (jrc < 0 || (jrc > 0 && steps == 0))
		{
			fprintf(stderr, "LinearSFM: -jgate: %s\n", jrc < 0 ? lsfm_last_error(ctx) : "pivots had to be floored (the information matrix is too close to singular)");
			return 3;
		}
		if (jrc > 0) fprintf(stderr, "LinearSFM: -jgate: the refinement took all %d steps and its last correction is still above the tolerance\n", steps);
	}
	const int r = 6 * out.m + 3 * out.n;
	if (!st.empty()) lsfm_save_state(st.c_str(), out.stVal, out.stno, r);
	if (!pose.empty() && !fea.empty()) lsfm_save_poses(pose.c_str(), fea.c_str(), out.stno, out.stVal, r); // only together (Imp.cpp:2078)
	if (!full.empty())
	{
		FILE* f = fopen(full.c_str(), "w");
		if (f) { for (int i = 0; i < r; i++) fprintf(f, "%d %.17g\n", out.stno[i], out.stVal[i]); fclose(f); }
	}
	if (!info.empty() && lsfm_write_localmap(info.c_str(), type, &out)) fprintf(stderr, "LinearSFM: cannot write %s\n", info.c_str());
	if (!fullbin.empty() && lsfm_save_state_bin(fullbin.c_str(), out.stVal, out.stno, r)) fprintf(stderr, "LinearSFM: cannot write %s\n", fullbin.c_str());
	if (!cov.empty() || !covf.empty())
	{
		// of the map the files above hold
		if (!covariances()) return 3;
		if (lsfm_save_covariances(cov.empty() ? nullptr : cov.c_str(), covf.empty() ? nullptr : covf.c_str(), out.stno, out.m, out.n, pc.data(), fc.data()))
			fprintf(stderr, "LinearSFM: cannot write the covariance files\n");
	}
	if (!covcols.empty())
	{
		// whole columns of the same map's covariance for the poses named by label
		std::vector<double> pc((size_t)q.size() * out.m * 36);
		int steps = 0; // (a positive status with no step taken: floored pivots, nothing written; with steps: the refinement ran out of them)
		const int crc = lsfm_map_covariance_columns(ctx, &out, type, q.data(), (int)q.size(), pc.data(), nullptr, nullptr, &steps, nullptr);
		if (crc < 0 || (crc > 0 && steps == 0))
		{
			fprintf(stderr, "LinearSFM: covariance columns: %s\n", crc < 0 ? lsfm_last_error(ctx) : "pivots had to be floored (the information matrix is too close to singular)");
			return 3;
		}
		if (crc > 0) fprintf(stderr, "LinearSFM: covariance columns: the refinement took all %d steps and its last correction is still above the tolerance\n", steps);
		if (lsfm_save_cov_columns(covcols.c_str(), out.stno, out.m, q.data(), (int)q.size(), pc.data())) fprintf(stderr, "LinearSFM: cannot write %s\n", covcols.c_str());
	}
	if (has_gate)
	{
		// the gate of the candidate pairs in the same map's covariance
		const int K = (int)gatepairs.size() / 2;
		std::vector<double> d2(K), cd((size_t)K * 9);
		int steps = 0;
		const int grc = lsfm_map_feature_pair_gate(ctx, &out, type, gatepairs.data(), K, d2.data(), cd.data(), &steps, nullptr);
		if (grc < 0 || (grc > 0 && steps == 0))
		{
			fprintf(stderr, "LinearSFM: gate: %s\n", grc < 0 ? lsfm_last_error(ctx) : "pivots had to be floored (the information matrix is too close to singular)");
			return 3;
		}
		if (grc > 0) fprintf(stderr, "LinearSFM: gate: the refinement took all %d steps and its last correction is still above the tolerance\n", steps);
		if (lsfm_save_pair_gate(gateout.c_str(), gateids.data(), K, d2.data(), cd.data())) fprintf(stderr, "LinearSFM: cannot write %s\n", gateout.c_str());
	}
	if (has_jgate)
	{
		const int K = (int)jgateids.size() / 2;
		if (lsfm_save_joint_gate(jgateout.c_str(), jgateids.data(), K, jstatus.data(), jd2.data(), jdelta.data(), jacc, jimp, jD2)) fprintf(stderr, "LinearSFM: cannot write %s\n", jgateout.c_str());
		if (has_jgatepairs)
		{
			std::vector<int> ids;
			for (int a = 0; a < K; a++)
				if (jstatus[a] == 1) { ids.push_back(jgateids[2 * a]); ids.push_back(jgateids[2 * a + 1]); }
			if (lsfm_save_pair_list(jgatepairs.c_str(), ids.data(), (long long)ids.size() / 2)) fprintf(stderr, "LinearSFM: cannot write %s\n", jgatepairs.c_str());
		}
	}
	if (has_mergeout)
	{
		const int K = (int)mergeids.size() / 2;
		std::vector<int> ids;
		for (int a = 0; a < K; a++) { ids.push_back(mergeids[2 * a]); ids.push_back(mergeids[2 * a + 1]); ids.push_back(mergekept[a]); }
		if (lsfm_save_merge_report(mergeout.c_str(), K, merge_removed, merge_dof, merge_d2, ids.data())) fprintf(stderr, "LinearSFM: cannot write %s\n", mergeout.c_str());
	}
	if (has_cand && lsfm_save_pair_list(cand.c_str(), candids.data(), ncand)) fprintf(stderr, "LinearSFM: cannot write %s\n", cand.c_str());
	if (!json.empty())
	{
		std::string cand_json = has_cand ? ", \"candidates\": " + std::to_string(ncand) : "";
		if (has_jgate)
		{
			char buf[160];
			snprintf(buf, sizeof buf, ", \"joint_gate\": {\"accepted\": %d, \"implied\": %d, \"D2\": %.17g}", jacc, jimp, jD2);
			cand_json += buf;
		}
		FILE* f = fopen(json.c_str(), "w");
		if (f)
		{
			fprintf(f, "{\"maps\": %d, \"type\": \"%s\", \"from_cache\": %s, \"poses\": %d, \"features\": %d, \"rc\": %d, \"t_total_ms\": %.6f, \"t_transform_ms\": %.6f, "
			           "\"t_join_ms\": %.6f, \"t_schur_ms\": %.6f, \"t_pcg_ms\": %.6f, \"t_backsub_ms\": %.6f, \"levels\": %d, \"joins\": %d, \"transforms\": %d, "
			           "\"pcg_iterations\": %ld, \"max_rel_residual\": %.6e, \"not_converged\": %d, \"attempts\": %d%s, "
			           "\"phases_s\": {\"read\": %.6f, \"context\": %.6f, \"upload\": %.6f, \"join_tree\": %.6f, \"download\": %.6f, \"write\": %.6f}}\n",
			        num, type ? "Monocular" : "Stereo", from_cache ? "true" : "false", out.m, out.n, rc, stats.t_total_ms, stats.t_transform_ms, stats.t_join_ms,
			        stats.t_schur_ms, stats.t_pcg_ms, stats.t_backsub_ms, stats.levels, stats.joins, stats.transforms, (long)stats.pcg_iterations,
			        stats.max_rel_residual, stats.not_converged, stats.attempts, cand_json.c_str(), w1 - w0, w2 - w1, w3 - w2, w4 - w3, w5 - w4, now() - w5);
			fclose(f);
		}
		else fprintf(stderr, "LinearSFM: cannot write %s\n", json.c_str());
	}
	if (!chi2f.empty())
	{
		// per-map chi2 of the state the files above hold (-robust: the polish's own, with its weights; otherwise weight 1)
		std::vector<int> dof(num);
		if (!chi2dof.empty()) dof = chi2dof;
		else if (chi2v.empty())
		{
			chi2v.resize(num);
			weightv.assign(num, 1.0);
			if (lsfm_map_chi2(ctx, maps.data(), num, type, &out, chi2v.data(), dof.data()) < 0) { fprintf(stderr, "LinearSFM: chi2: %s\n", lsfm_last_error(ctx)); return 3; }
		}
		else
			for (int k = 0; k < num; k++) dof[k] = 6 * maps[k].m + 3 * maps[k].n;
		FILE* f = fopen(chi2f.c_str(), "w");
		if (f)
		{
			for (int k = 0; k < num; k++) fprintf(f, "%d %d %.17g %.17g\n", k + 1, dof[k], chi2v[k], weightv[k]);
			fclose(f);
		}
		else fprintf(stderr, "LinearSFM: cannot write %s\n", chi2f.c_str());
	}
	if (!chi2ff.empty())
	{
		// per-feature chi2 of the same state (-robustf: the polish's own, with its weights; otherwise weight 1), through a temporary file
		if (fchi2v.empty())
		{
			fchi2v.resize(nfeat + 1); fweightv.assign(nfeat + 1, 1.0);
			if (lsfm_map_feature_chi2(ctx, maps.data(), num, type, &out, fchi2v.data(), nullptr) < 0) { fprintf(stderr, "LinearSFM: chi2f: %s\n", lsfm_last_error(ctx)); return 3; }
		}
		const std::string tmp = chi2ff + ".tmp";
		FILE* f = fopen(tmp.c_str(), "w");
		bool ok = f != nullptr;
		if (f)
		{
			size_t q = 0;
			for (int k = 0; k < num; k++)
				for (int i = 0; i < maps[k].n; i++, q++)
					ok = fprintf(f, "%d %d %.17g %.17g\n", k + 1, maps[k].stno[6 * maps[k].m + 3 * i], fchi2v[q], fweightv[q]) > 0 && ok;
			ok = fclose(f) == 0 && ok;
		}
		if (!ok || rename(tmp.c_str(), chi2ff.c_str()) != 0) { fprintf(stderr, "LinearSFM: cannot write %s\n", chi2ff.c_str()); remove(tmp.c_str()); }
	}
	if (want_stats)
		fprintf(stderr, "lsfm_e2e: read %.3f s, context %.3f s, upload %.3f s, join tree %.3f s, download %.3f s, write %.3f s\n", w1 - w0, w2 - w1, w3 - w2,
		        w4 - w3, w5 - w4, now() - w5);
	lsfm_map_release(&out);
	for (auto& g : maps) lsfm_map_release(&g);
	lsfm_context_destroy(ctx);
	return partial ? 4 : 0;
}
