// The Gauss-Newton polish's joint system, the part that depends on labels and index arrays alone: which global variable every local one
// is, where every local block lands in the joint U / W, the gauge, the correction slots of the feature weights and the coalesced form of
// lsfm_gn_linearise.  Plain C++ (lsfm_gn_structure.cpp, compiled by g++ like lsfm_marg_poses.cpp: callable without a device; C ABI:
// lsfm_gn_structure); the upload and the numbers are lsfm_gn.hip / lsfm_gn_assemble.hip / lsfm_gn_chi2.hip.
#pragma once
#include <string>
#include <vector>

struct lsfm_map;

namespace lsfm {

// one local map's place in the uploaded batch and in the joint system (the structural head of the device's GnMap)
struct GnMapShape {
	int nh;           // hub columns: 0 = the map's frame is the global frame (Stereo, Ref_k == the global Ref), 1 Stereo, 2 Mono
	int hub[2];       // global pose of Ref_k [, ScaP_k]
	int fix;          // Mono: Fix_k
	int p0, m, f0, n; // its poses / features in the uploaded batch
	int u0, nu;       // its blocks in the U list the assembly reads: nu_own blocks of its own, then its correction slots (if any)
	int nu_own;       // the map's own U blocks: what I_k holds
	int ubase;        // its first block in the joint U: nh * m blocks (a, h_s), nh (nh + 1) / 2 blocks (h_s, h_t), nu blocks
};
// The correction slots of the feature weights: per map one slot per distinct pair (a <= b, local poses) of poses that see a common
// feature, sorted by (a, b); per slot its contributors in feature order.  And the extended U list: every map's own blocks, then its slots.
struct GnSlots {
	std::vector<int> before;            // [N + 1] slots ahead of map k
	std::vector<int> a, b;              // [NS] the slot's local poses
	std::vector<int> sptr, cf, ca, cb;  // contributors of slot s: sptr[s] .. sptr[s + 1]; feature instance, entries of a and of b
	std::vector<int> eptr, eidx;        // entry e = one (feature instance, pose): its W blocks eidx[eptr[e] .. eptr[e + 1]) (batch indices)
	std::vector<int> Uix, Ujx, sdst;    // [NU + NS] batch poses of the extended list's blocks; [NS] the slot's block in it
	std::vector<int> ushift;            // [N] own block i of map k is block i + ushift[k] of the extended list
};
// lsfm_gn_linearise: the joint system with every block once.  Output W sorted by feature, within a feature by pose; output U sorted by
// (i, j); per output block its sources in the joint W / U as a CSR (wsp / wsi, usp / usi), in source (= map) order.
struct GnCoalesced {
	int nWo = 0, nUo = 0;
	std::vector<int> photo, feature, FBlock, Ui, Uj, wsp, wsi, usp, usi;
};
struct GnStructure {
	int N = 0, M = 0, NFG = 0, P = 0, FI = 0, NUJ = 0, NWJ = 0; // maps; global poses, features; local poses, features; joint U, W blocks
	bool mono = false, has_slots = false, has_coalesced = false;
	std::vector<int> pose_off, feat_off, u_off, w_off; // [N + 1] prefix sums of m, n, nU, nW: the batch's offsets
	std::vector<GnMapShape> map;                       // [N]
	std::vector<int> dof;                              // [N] 6 m_k + 3 n_k
	std::vector<int> gp, gf;                           // [P] / [FI] global variable of a local pose / feature
	std::vector<int> wdst;                             // [FI] first joint W block of the instance: its nh hub blocks, then its own run
	std::vector<int> fptrJ, photoJ;                    // [NFG + 1] / [NWJ] the joint W: per global feature its instances in map order
	std::vector<int> fsp, fsi, psp, psi;               // CSRs: the instances of a global feature; of a global pose: instances (>= 0) and hub roles (-1 - (2 map + s))
	std::vector<int> UiJ, UjJ;                         // [NUJ] joint U coordinates (row <= column)
	std::vector<int> origin;                           // [M] x->pose_origin, or the first map that holds the pose
	std::vector<unsigned char> fixed;                  // Mono: [6 M + 3 NFG] 1 = a gauge scalar; Stereo: empty
	GnSlots sl;                                        // has_slots (without: sl.before alone, all 0)
	GnCoalesced co;                                    // has_coalesced
};

// LSFM_OK, or LSFM_ERR_ARG with `why` for what cannot be placed.  The maps' index arrays must be valid already (the device calls: batch_upload
// has checked them; lsfm_gn_structure: system_check).  want_slots: every map's U range is extended by its correction slots.
int gn_structure(const lsfm_map* maps, int N, bool mono, const lsfm_map* x, bool want_slots, bool want_coalesce, GnStructure& st, std::string& why);

} // namespace lsfm
