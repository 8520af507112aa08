// Marginalising poses out of a map (lsfm_map_marginalise_poses): the part that depends on labels and flags alone.  Plain C++
// (lsfm_marg_poses.cpp, compiled by g++ like lsfm_system.cpp / lsfm_symbolic.cpp: callable without a device); the numbers are
// lsfm_marg_poses.hip (declared in lsfm_marg.hpp).
#pragma once
#include <string>
#include <vector>

struct lsfm_map;

namespace lsfm {

// D: the dropped poses, K: the kept ones, U1: the map's U after its dropped features are gone (canonical: one block per pair).
// Pose indices are the INPUT map's unless said otherwise; every list ascends.
struct PoseMargStructure {
	int m = 0, ncomp = 0;
	std::vector<int> dlist, klist; // D and K
	std::vector<int> local;        // [m] position of a pose in dlist (dropped) or in klist (kept: its index in the output map)
	std::vector<int> comp;         // [m] connected component of a dropped pose in the graph of U1_DD, numbered by their smallest pose; kept: -1
	std::vector<int> nptr, nidx;   // CSR [ncomp + 1]: N(c), the kept poses with a block of U1 into component c
	std::vector<int> bd;           // Bd = the union of all N(c)
	std::vector<int> bdpos;        // [m] position in bd, -1: not a boundary pose
	// U' in the output's numbering, sorted by (Ui, Uj) -- the diagonal block leads its row: the pairs of U1_KK, the fill pairs (both in
	// N(c) of one component) and every diagonal
	std::vector<int> oUi, oUj;
	std::vector<int> osrc;         // block of U1 the pair has, -1: fill alone
	std::vector<char> ofill;       // 1: a fill pair
};

// The flags of the features stage A drops.  Rules: the Ref pose (Mono: the ScaP pose too), where it is in the state, is kept; a
// feature seen by a dropped pose is dropped -- drop_feat == null: exactly those, otherwise the caller's flags, which must cover them.
// LSFM_OK, or LSFM_ERR_ARG with `why`.
int pose_marg_flags(const lsfm_map* map, bool mono, const unsigned char* keep_pose, const unsigned char* drop_feat, std::vector<unsigned char>& drop,
                    std::string& why);
// The sorted, distinct pairs (Ui << 32 | Uj) of stage A's result without a device: the pairs of U, the pairs of poses that see a common
// dropped feature, every diagonal (fptr: the W run of every feature, system_check)
std::vector<unsigned long long> marg_pattern_host(const lsfm_map* map, const std::vector<int>& fptr, const unsigned char* drop);
// components, boundaries and the pattern of U' from the pattern of U1 (nU blocks, Ui <= Uj, no pair twice)
void pose_marg_structure(int m, int nU, const int* Ui, const int* Uj, const unsigned char* keep_pose, PoseMargStructure& st);

} // namespace lsfm
