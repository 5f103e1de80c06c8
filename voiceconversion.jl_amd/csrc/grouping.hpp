// grouping.hpp -- the stable counting sort of frames by an integer key (gmmmap_group.hip), as gmmmap.hip and estep.hip use it.
#pragma once
#include "vcmi_common.hpp"

struct vcmi_gmmmap;

namespace vcmi {
constexpr int kGroupChunk = 1024;     // frames per chunk of the grouping sort (64 tiles of 16; 16 wave rows of 64)

// ---- fvconvert and predict (gmmmap.hip): frames grouped by their nearest source mean, in two launches (keys with chunk and
// super-chunk histograms, then gmmmap_group_place_kernel: no scan) ----
// whether a call of T frames on g can be grouped at all (enough frames, a key operand, its LDS)
bool can_group(const vcmi_gmmmap *g, int64_t T);
// The two grouping kernels on g's scratch: *perm_out = frames in group order, *gbase_out = first sorted position of every group
// (M + 1 ints), *key_out = group of every frame.  Enters g->grp_order on st; the caller leaves it after its last kernel.
int launch_grouping(vcmi_gmmmap *g, const double *dX, int64_t ldx, int64_t T, hipStream_t st, int **key_out, int **perm_out,
                    int **gbase_out);

// ---- the E-step's hard path (estep.hip): the scan + scatter pair, launched behind its gate ----
// chunkhist[c][k] (counts of key k in chunk c of kGroupChunk consecutive frames) -> its exclusive prefix over the chunks, total[k]
// (gate, optional: a device word; 0 -> the kernel returns at once -- estep_path.hpp)
__global__ void gmmmap_group_scan_kernel(int *__restrict__ chunkhist, int64_t nchunks, int M, int *__restrict__ total, const int64_t *__restrict__ gate);
// perm: frames in key order, inside a key in frame order (needs (17 * M) ints of dynamic LDS, one workgroup of 256 per chunk)
__global__ void gmmmap_group_scatter_kernel(const int *__restrict__ key, int64_t T, int M, const int *__restrict__ chunkhist,
                                            const int *__restrict__ total, int *__restrict__ perm, const int64_t *__restrict__ gate);
}  // namespace vcmi
