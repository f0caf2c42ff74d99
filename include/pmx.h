/*
 * pmx.h - C ABI of the MI355X screening engine (libpmx.so, built from pharmaconet_amd/csrc).
 *
 * The reference (SeonghwanSeo/PharmacoNet, /root/reference) has no FFI for this path; its seams are
 * Python-level. Each entry point below names the reference interface it stands in for (paths are
 * relative to /root/reference). The Python shim that binds these symbols is
 * pharmaconet_amd/_ffi.py; the stub a reference maintainer would add is shown in INTEGRATION.md.
 *
 * Conventions: every function returns 0 on success and a non-zero pmx_status otherwise;
 * pmx_last_error() gives the calling thread's last message. No exceptions cross the boundary.
 * Handles are opaque; a handle is bound to the device it was created on. Every entry point may be called from
 * any thread. pmx_score / pmx_score_multi keep their work buffers per (device, stream): calls on different streams run
 * concurrently, calls on the same stream are ordered by it (a second host thread enqueuing on the same stream waits for
 * the first to finish enqueuing, not for the GPU). `stream` is a hipStream_t
 * passed as void* (NULL = the default stream). Pointers named *_dev are device pointers on that device.
 */
#ifndef PMX_H
#define PMX_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMX_NUM_TYPES 7          /* Hydrophobic, Aromatic, Cation, Anion, HBond_donor, HBond_acceptor, Halogen */
#define PMX_MAX_LEVELS 20        /* src/pmnet/scoring/graph_match.py:88 */
#define PMX_MAX_MODEL_NODES 256   /* node sets are lists on the device; cluster_nodes is a bit mask of ceil(n_nodes / 64) words */
#define PMX_MAX_MODEL_CLUSTERS 128 /* candidate sets of a ligand cluster are two 64-bit words */
#define PMX_MAX_LEVEL_CANDIDATES 64 /* model clusters that share a type with ONE ligand cluster (a tree level's candidates): a ligand
                                       with a cluster beyond that is reported PMX_LIGAND_UNSUPPORTED (only models of more than 64 clusters can do that) */
#define PMX_MAX_LIGAND_NODES 64
#define PMX_MAX_LIGAND_CLUSTERS 64
#define PMX_MAX_CONFORMERS 64

typedef enum {
    PMX_OK = 0,
    PMX_ERR_INVALID = 1, /* bad argument / model or library outside the structural limits above */
    PMX_ERR_HIP = 2,     /* a HIP runtime call failed */
    PMX_ERR_OOM = 3
} pmx_status;

/* Per-ligand status written by pmx_score. */
#define PMX_LIGAND_OK 0
#define PMX_LIGAND_UNSUPPORTED 1 /* record exceeds a structural limit; score is NaN */
#define PMX_LIGAND_TOO_LARGE 2   /* the ligand's score tables exceed the whole table arena (PMX_ARENA_MB); score is NaN */
#define PMX_LIGAND_EXPLAIN_MISS 3 /* pmx_explain: a conformer's maximum was not met by any leaf (reserved: the explain walker records the
                                     leaf that sets each maximum, so it cannot occur; a caller that sees it has found a bug) */
#define PMX_LIGAND_KEY_INVALID 4  /* pmx_attribute: the row's conformer or key is not one of the ligand's tree (see there); total and node shares are NaN */

typedef struct pmx_model pmx_model;
typedef struct pmx_library pmx_library;

/*
 * Flat pharmacophore model: the object graph built by PharmacophoreModel.__setstate__
 * (src/pmnet/pharmacophore_model.py:191-204) made positional. edge_mean / edge_std are the
 * float32 values of `model_node1.neighbor_edge_dict[model_node2].distance_mean / .distance_std`
 * (src/pmnet/scoring/match_utils.py:35-48) for every ordered node pair, self-loops included.
 * The matrices need not be symmetric: a term of ligand nodes (u, v) reads edge [m * n_nodes + n], m matched to u and n to v, with u before v
 * in its cluster's order (self entries) or u in the cluster of the earlier tree level (pair entries), as oracle/pmx_oracle.c node_pair_term.
 * Clusters are listed in `model.node_clusters` order (pharmacophore_model.py:202-204);
 * cluster_typemask is the stored `node_types` set, cluster_center / cluster_size feed the
 * cluster-distance prefilter (src/pmnet/scoring/graph_match.py:263-268).
 * All pointers are host pointers; the data is copied.
 */
typedef struct {
    int32_t n_nodes;
    int32_t n_clusters;
    const uint8_t *node_type;        /* [n_nodes] type id 0..6 */
    const float *edge_mean;          /* [n_nodes * n_nodes] */
    const float *edge_std;           /* [n_nodes * n_nodes] */
    const uint64_t *cluster_nodes;   /* [n_clusters * W], W = max(1, ceil(n_nodes / 64)): bit (m % 64) of word a * W + m / 64 = node m belongs
                                        to cluster a (one word per cluster for models of up to 64 nodes) */
    const uint8_t *cluster_typemask; /* [n_clusters] */
    const double *cluster_center;    /* [n_clusters * 3] */
    const double *cluster_size;      /* [n_clusters] */
} pmx_model_desc;

/*
 * Packed ligand library (format: pharmaconet_amd/library.py): what GraphMatcher reads from each
 * ligand's LigandGraph (src/pmnet/scoring/ligand.py:110-259) - typed nodes, per-conformer node
 * positions, clusters in priority_fn order (graph_match.py:43-60). Replaces the per-file
 * `Ligand.load_from_file` objects that screening.py:46-47 hands to scoring_file one at a time.
 */
typedef struct {
    uint64_t n_ligands;
    const uint64_t *offsets; /* [n_ligands + 1] byte offsets into data, each a multiple of 16 */
    const uint8_t *data;
    int32_t on_device;       /* 0: host pointers (copied to the device); 1: device pointers (copied device-to-device); 2: device pointers, ADOPTED - the library
                                reads the caller's buffers in place (no allocation, no copy: what pmx_pack_features_device wrote, as it lies); they must
                                stay valid and unchanged until pmx_library_destroy, which does not free them. A device view must be complete when the call
                                is made (the call reads it on the default stream). */
} pmx_library_view;

typedef struct {
    uint64_t n_ligands;
    uint64_t n_bytes;
    uint64_t total_conformers;
    int32_t max_nodes, max_conformers, max_clusters;
    int32_t n_unsupported;
} pmx_library_info;

const char *pmx_last_error(void);
int pmx_version(void);

/* PharmacophoreModel.load (pharmacophore_model.py:163-176) -> device-resident tables. */
int pmx_model_create(const pmx_model_desc *desc, int device, pmx_model **out);
int pmx_model_destroy(pmx_model *model);

int pmx_library_upload(const pmx_library_view *view, int device, pmx_library **out);
int pmx_library_info_get(const pmx_library *lib, pmx_library_info *info);
int pmx_library_destroy(pmx_library *lib);

/*
 * Batched PharmacophoreModel._scoring (pharmacophore_model.py:101-106), i.e.
 * GraphMatcher(model, ligand, weights).run() (graph_match.py:94-101) for ligands
 * [first, first + count). weights[7] = DEFAULT_WEIGHTS updated by the caller's dict
 * (graph_match.py:32-40,81-83) in type-id order. scores_dev[count] receives the float32 value
 * of the float the reference returns (0 for ligands without clusters or candidates,
 * graph_match.py:95-99); status_dev[count] (may be NULL) receives PMX_LIGAND_*.
 * Everything is enqueued and the call returns: no device-to-host read, no synchronisation, no helper thread (a
 * synchronisation happens only when a cached work buffer has to grow). The work is ordered on `stream`: per chunk of ligands
 * (PMX_SUPER) the ligand kernel (score tables in per-wavefront slices + tree search within a pass budget), the same for
 * ligands with larger tables, a fixed number of task rounds for the subtrees of over-budget trees, finalize - one in-order
 * sequence on `stream`, no other stream, no event to wait for. Work buffers are kept per (device, stream) for at most PMX_MAX_WORKSPACES (default 4) streams per device - the least recently used idle workspace is
 * freed when one more stream appears. At the defaults: about 73 GB for libraries of up to 8 conformers and an 11-cluster model (64 GB table arena,
 * 2 GB task queue, <= 4 GB large slices, 0.7 GB slices, 1.8 GB path sums), about 70 GB at 32 / 64 conformer lanes (32 GB arena, 8 GB queue, <= 16 GB
 * large slices, slices that grow with the square of the model's cluster count); PMX_ARENA_MB, PMX_TASKQ_MB size the arena and
 * the queue of a workspace. Without PMX_ARENA_MB the table arena takes at most a third of the device memory that is free when it is first allocated, and it shrinks when device memory is short - a smaller arena is slower, never
 * wrong - and keeps the size it got until pmx_release_workspaces. PMX_LIGAND_TOO_LARGE is reported for a ligand whose tables exceed a whole
 * arena; a ligand that merely found the arena full of other ligands' tables is taken again with the arena empty, in up to PMX_ARENA_RETRIES
 * (default 4) further passes (only models whose largest possible tables exceed a large slice have such passes).
 */
int pmx_score(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], uint64_t first,
              uint64_t count, float *scores_dev, int32_t *status_dev, void *stream);

/*
 * pmx_score with the score as a float64: the value `GraphMatcher.run()` returns is `float(np.mean(...))` of float64 per-conformer maxima
 * (graph_match.py:103-109); pmx_score rounds it to float32, this entry point hands it over as it is (scores_dev = double[count]), so that a
 * CSV written from it (screening.py:70-75) carries the reference's digits as far as the tabulated pair functions allow (relative 1e-7) and
 * two ligands closer than a float32 ulp keep the order the float64 values give them. Same work, same kernels.
 */
int pmx_score_f64(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], uint64_t first,
                  uint64_t count, double *scores_dev, int32_t *status_dev, void *stream);
int pmx_score_multi_f64(const pmx_model *const *models, int n_models, const pmx_library *lib,
                        const float weights[PMX_NUM_TYPES], uint64_t first, uint64_t count, double *scores_dev,
                        int32_t *status_dev, void *stream);

/* The same for several models over one library: the pockets' chunks are one sequence of one call, one pocket after the other
 * on `stream`;
 * scores_dev is [n_models][count], status_dev[count] is written once. */
int pmx_score_multi(const pmx_model *const *models, int n_models, const pmx_library *lib,
                    const float weights[PMX_NUM_TYPES], uint64_t first, uint64_t count, float *scores_dev,
                    int32_t *status_dev, void *stream);

/*
 * The ranking step of screening.py:70 (`result.sort(key=score, reverse=True)`, stable): the k best
 * of scores_dev[n] in descending score order, ties in ascending index order. -0.0 and +0.0 are one value (they tie; each is
 * reported as given). index_dev may be
 * NULL (element i has index base_index + i) or give each element's global index.
 * out_scores_dev[k], out_index_dev[k]; if n < k the tail is filled with -inf / UINT64_MAX. A NaN score (an unsupported ligand)
 * ranks after every real score and is reported as NaN with its index; input elements whose index is UINT64_MAX are padding
 * (they rank last). k <= 65536, n < 2^31. A radix select on the device (csrc/pmx_topk.hip): no sort of all n, no library.
 */
int pmx_topk(const float *scores_dev, const uint64_t *index_dev, uint64_t n, uint64_t base_index, int k,
             float *out_scores_dev, uint64_t *out_index_dev, int device, void *stream);

/*
 * Multi-GPU exchange (one process per GPU). Replaces the gather-and-sort of screening.py:66-70 (`pool.map` over all
 * files, then one Python sort): every rank scores a contiguous shard, takes its k best with pmx_topk (global indices:
 * base_index = first ligand of the shard) and calls pmx_topk_allgather, which all-gathers the (score, index) lists
 * over RCCL (xGMI inside a node) and merges them identically on every rank - descending score, ties by ascending
 * global index. The communicator is built from an id made on rank 0 (pmx_comm_unique_id) and handed to the other
 * ranks by the host program (file, socket, torch.distributed store ...).
 */
#define PMX_COMM_ID_BYTES 128
typedef struct pmx_comm pmx_comm;
int pmx_comm_unique_id(char id_out[PMX_COMM_ID_BYTES]);
int pmx_comm_create(const char id[PMX_COMM_ID_BYTES], int rank, int nranks, int device, pmx_comm **out);
int pmx_comm_info(pmx_comm *comm, int *rank_out, int *nranks_out, int *device_out); /* as RCCL reports them (ncclCommCount / UserRank / CuDevice) */
int pmx_comm_destroy(pmx_comm *comm);
int pmx_topk_allgather(pmx_comm *comm, const float *scores_k_dev, const uint64_t *index_k_dev, int k, float *out_scores_dev,
                       uint64_t *out_index_dev, void *stream);

/*
 * The library packer in native code (pmx_pack.cpp): what LigandGraph.__init__ (src/pmnet/scoring/ligand.py:110-259) and the
 * priority sort of graph_match.py:43-60 make of a molecule's perceived pharmacophore features, as records of the packed
 * library format. Input = what Ligand.__init__ hands to LigandGraph (ligand.py:16-61,120-132), flat over a batch of
 * molecules: per atom its atomic number and heavy-atom neighbours (CSR, in the order OBAtomAtomIter yields them); per
 * feature (`pharmacophore_list` order, ligand_utils.py:80-88) its type id, the atom indices and the centre indices, with
 * flags bit 0 / bit 1 telling whether atom_indices / center_indices was a tuple rather than an int (an int and a
 * 1-tuple are different node keys, ligand.py:137); positions float32 [n_atoms][n_conformers][3] per molecule.
 * offsets_out[n_mols + 1] and data_out receive the library; *data_bytes the bytes written. Sizing: a call with data_out =
 * NULL packs nothing and returns in *data_bytes an upper bound (every feature a node) - allocate that, pack once, keep the
 * first *data_bytes bytes. With a data_cap that turns out too small the call fails and *data_bytes holds the exact need.
 * status_out (may be NULL): 1 for a molecule outside the structural limits above, 2 for malformed input (type id above 6, an atom /
 * centre / neighbour index outside the molecule, a feature without atoms, too few positions) or a feature graph on which the
 * reference's builder raises (a dependent node whose ring has no cluster); either becomes a header-only record that pmx_score
 * reports as PMX_LIGAND_UNSUPPORTED. Offsets that run backwards fail the whole call.
 */
typedef struct {
    uint64_t n_mols;
    const uint64_t *atom_off;        /* [n_mols + 1] first atom of each molecule */
    const uint8_t *atomic_num;       /* [total atoms] */
    const uint64_t *nbr_off;         /* [total atoms + 1] */
    const int32_t *nbr;              /* neighbour atom indices, local to the molecule */
    const uint64_t *feat_off;        /* [n_mols + 1] first feature of each molecule */
    const uint8_t *feat_type;        /* [total features] type id 0..6 */
    const uint8_t *feat_flags;       /* [total features] bit 0: atom_indices is a tuple, bit 1: center_indices is a tuple */
    const uint64_t *feat_atom_off;   /* [total features + 1] */
    const int32_t *feat_atoms;
    const uint64_t *feat_center_off; /* [total features + 1] */
    const int32_t *feat_centers;
    const int32_t *n_conf;           /* [n_mols] */
    const uint64_t *pos_off;         /* [n_mols + 1] float offset of each molecule's positions */
    const float *positions;
} pmx_feature_batch;
int pmx_pack_features(const pmx_feature_batch *batch, int threads, uint64_t *offsets_out, uint8_t *data_out, uint64_t data_cap,
                      uint64_t *data_bytes, int32_t *status_out);
/*
 * The same packer on the device (pmx_pack_device.hip), for batches that are in device memory: every pointer of `batch`, offsets_out,
 * data_out and status_out are DEVICE pointers; the struct itself and data_bytes are on the host. Records are byte-identical to
 * pmx_pack_features'. The kernels run on `stream` (a hipStream_t; NULL = the default stream) and the call waits for the sizes (one
 * 8-byte read) before it enqueues the record writer and returns: *data_bytes is the exact size, offsets_out and data_out are
 * complete in stream order. A call with data_out = NULL only sizes (EXACTLY, unlike the host call's bound; the bound
 * sum(((8 + 2 nf + 3 + 12 nf c + 15) & ~15) + 16) over the molecules' feature and conformer counts needs no call at all).
 * Calls share one set of work buffers per process: they are serialised on the host, and a call made on another stream than the one before
 * it starts, on the device, behind that call's record writer.
 * status_out as above, plus 3: the molecule is outside the fixed scratch of the device builder (more than 256 atoms, 255 features,
 * 1024 neighbour entries, 1024 feature-atom entries, or a feature of more than 16 atoms) and became a header-only record - pack
 * such a batch with pmx_pack_features. Two differences in reporting, none in records: a molecule whose offsets run backwards is
 * reported 2 (the host call fails as a whole), and a molecule of more than 64 nodes is reported 1 without looking further (the host
 * packer reports 2 if the reference's builder would also raise on it).
 */
int pmx_pack_features_device(const pmx_feature_batch *batch, int device, void *stream, uint64_t *offsets_out, uint8_t *data_out,
                             uint64_t data_cap, uint64_t *data_bytes, int32_t *status_out);

/*
 * A sub-library on the device (pmx_select.hip): the records of the listed ligands, gathered into a new library without leaving HBM.
 * The reference has no counterpart - its library is a list of files, and a list of hits is a Python slice of it (screening.py:66-75);
 * here it is what turns "the best 10^5 hits", "the survivors of a filter" or "these hits, for the next campaign" back into something
 * pmx_score / pmx_score_multi take, which score a contiguous range and nothing else.
 *   indices_dev[n]        library indices, any order, repeats allowed; record i of the new library is a byte copy of record indices_dev[i]
 *   offsets_out_dev       uint64 [n + 1], written in full by every call that gets as far as the device (offsets_out_dev[0] = 0)
 *   data_out_dev          the records; data_cap its size in bytes. Must not overlap the source library's buffers (PMX_ERR_INVALID)
 *   *data_bytes           (host) the exact size of the new library's data
 * The conventions are pmx_pack_features_device's: the kernels run on `stream`, the host waits once - for one 24-byte read: the total and
 * the count and first position of indices outside the library - and the record copy is enqueued behind it; offsets_out_dev and
 * data_out_dev are complete in stream order. A call with data_out_dev = NULL only sizes (offsets and *data_bytes; data_cap must be 0);
 * a call with data_out_dev does the same and then copies; with a data_cap that is too small it fails with PMX_ERR_INVALID, *data_bytes
 * holds the need and nothing is copied. An index >= n_ligands fails the call with PMX_ERR_INVALID - the message gives how many there
 * are and the first position that holds one - and no record is written (*data_bytes is 0). n = 0 succeeds: offsets_out_dev[0] = 0,
 * *data_bytes = 0. n > 2^31 - 1 is PMX_ERR_INVALID (the scan's limit, as in pmx_pack_features_device). The source may be a library of
 * any origin (uploaded, copied on the device, adopted); the new buffers are the caller's - pmx_library_upload with on_device = 2 makes
 * them a library. Work buffers (8 bytes per index, the scan's scratch, three counters) are kept per device, grow only when a call needs
 * more, are shared by calls on all streams (a call holds them until its host wait has ended) and are freed by pmx_release_workspaces.
 */
int pmx_library_select(const pmx_library *lib, const uint64_t *indices_dev, uint64_t n, uint64_t *offsets_out_dev /* [n + 1] */,
                       uint8_t *data_out_dev, uint64_t data_cap, uint64_t *data_bytes, void *stream);
/* The device buffers a library reads (owned, copied or adopted) - offsets uint64 [n_ligands + 1], data [n_bytes] - for reading it back.
 * Valid until pmx_library_destroy (an adopted library's for as long as their owner keeps them); not to be written to. */
int pmx_library_buffers(const pmx_library *lib, const uint64_t **offsets_dev, const uint8_t **data_dev);

/*
 * The rule half of ligand perception in native code (pmx_perceive.cpp): get_pharmacophore_nodes of
 * src/pmnet/scoring/ligand_utils.py:25-184 for a batch of molecules. The reference asks OpenBabel per atom inside Python
 * predicates, one molecule at a time; here what only the chemistry toolkit can say comes in as flat per-atom answers, taken on the
 * hydrogen-free molecule (pybel `removeh()`, ligand.py:37-38) in atom order:
 *   atomic_num        OBAtom::GetAtomicNum            explicit_degree  GetExplicitDegree        heavy_degree  GetHvyDegree
 *   hyb               GetHyb                          h_count          explicit hydrogens still bound to the atom (0 after removeh)
 *   flags             bit 0: IsHbondAcceptor; bit 1: IsHbondDonor of the same atom after AddPolarHydrogens on a copy (ligand_utils.py:30-34,46)
 *   nbr_off / nbr     heavy-atom neighbours (CSR over all atoms of the batch; indices local to the molecule) in OBAtomAtomIter order
 *   ring_off / ring_atom_off / ring_atoms   the AROMATIC rings of the SSSR (pybel `sssr`, `ring.IsAromatic()`), atoms in any order
 * Output: the molecules' feature lists in pharmacophore_list order (ligand_utils.py:80-88) in the layout of pmx_feature_batch
 * (feat_off[n_mols + 1], feat_type, feat_flags, feat_atom_off, feat_atoms, feat_center_off, feat_centers) - together with the atom arrays
 * above and the conformer coordinates that IS the input of pmx_pack_features. A call with feat_type == NULL only counts (*n_features,
 * *n_feat_atoms, *n_feat_centers and feat_off are written). status_out (may be NULL): 2 for a molecule with malformed input (a neighbour
 * or ring atom outside the molecule), which gets no features.
 */
typedef struct {
    uint64_t n_mols;
    const uint64_t *atom_off;      /* [n_mols + 1] first atom of each molecule */
    const uint8_t *atomic_num;     /* [total atoms] */
    const uint8_t *explicit_degree;
    const uint8_t *heavy_degree;
    const uint8_t *hyb;
    const uint8_t *h_count;
    const uint8_t *flags;
    const uint64_t *nbr_off;       /* [total atoms + 1] */
    const int32_t *nbr;
    const uint64_t *ring_off;      /* [n_mols + 1] first aromatic ring of each molecule */
    const uint64_t *ring_atom_off; /* [total rings + 1] */
    const int32_t *ring_atoms;     /* atom indices local to the molecule */
} pmx_atom_batch;
int pmx_perceive_features(const pmx_atom_batch *batch, int threads, uint64_t *feat_off, uint8_t *feat_type, uint8_t *feat_flags,
                          uint64_t *feat_atom_off, int32_t *feat_atoms, uint64_t *feat_center_off, int32_t *feat_centers,
                          uint64_t cap_features, uint64_t cap_atoms, uint64_t cap_centers, uint64_t *n_features, uint64_t *n_feat_atoms,
                          uint64_t *n_feat_centers, int32_t *status_out);

/*
 * Conformer coordinates of an SD file in native code: the coordinate half of Ligand.load_from_file
 * (src/pmnet/scoring/ligand.py:63-84), which has OpenBabel build a molecule object per record and copies
 * `[atom.coords for atom in pbmol.atoms]` in a Python loop after removeh(). The features come from the first record alone
 * (ligand.py:78-84), so the further records only contribute heavy-atom coordinates: element and float32 position of every
 * atom that is not a hydrogen (H, D, T), in file order, record after record (MDL molfile V2000 and V3000, records separated
 * by $$$$). `text` / `len`: the file's bytes. max_records: records to read (num_conformers; 0 = all). With atomic_num ==
 * NULL and xyz == NULL the call only counts (*n_records, *n_atoms). A record that cannot be parsed fails the call with
 * PMX_ERR_INVALID and leaves its index in *n_records.
 */
int pmx_sdf_heavy_atoms(const char *text, uint64_t len, uint64_t max_records, uint64_t cap_records, uint64_t cap_atoms,
                        uint64_t *n_records, uint64_t *n_atoms, int32_t *atoms_per_record, uint8_t *atomic_num, float *xyz);

/*
 * The same for a Tripos mol2 file (`pybel.readfile("mol2", ...)` in ligand.py:72): every @<TRIPOS>MOLECULE record's
 * @<TRIPOS>ATOM section, the element taken from the SYBYL atom type in front of its dot, hydrogens dropped. An atom type that
 * names no element (Du, LP, Any ...) fails the call with PMX_ERR_INVALID like any record it cannot parse: the caller then
 * reads the file the reference's way.
 */
int pmx_mol2_heavy_atoms(const char *text, uint64_t len, uint64_t max_records, uint64_t cap_records, uint64_t cap_atoms,
                         uint64_t *n_records, uint64_t *n_atoms, int32_t *atoms_per_record, uint8_t *atomic_num, float *xyz);

/*
 * Voxel components of hotspot density maps on the device - the search of `DensityMapGraph.__extract_pharmacophores`
 * (src/pmnet/utils/density_map.py:78-110) that `PharmacophoreModel.create` (pharmacophore_model.py:108-149) runs per hotspot in a
 * Python loop over 26 neighbours per voxel. `maps`: n_maps arrays float32 [size][size][size] (C order, mask[x][y][z]); a voxel is
 * in a component where its value is > 0; voxels are named by their linear index (x * size + y) * size + z.
 *   pmx_density_create  uploads the maps and labels the 26-connected components (label = smallest linear index of the component);
 *   pmx_density_labels  labels_out [n_maps * size^3], -1 outside the components;
 *   pmx_density_order   for n_components components (map, seed voxel, offset into members_out; sizes from the labels): the voxels in
 *                       the order the reference's breadth-first search from that seed discovers them (:93-109: the member list is the
 *                       queue, neighbours in itertools.product((-1, 0, 1), repeat=3) order) - the order of its centroid sums. The seed
 *                       of a search is `set.pop()` on a CPython set (:91-92): the caller's business (pharmaconet_amd/model_builder.py).
 */
typedef struct pmx_density pmx_density;
int pmx_density_create(const float *maps, int32_t n_maps, int32_t size, int device, pmx_density **out);
int pmx_density_labels(pmx_density *d, int32_t *labels_out);
int pmx_density_order(pmx_density *d, int32_t n_components, const int32_t *comp_map, const int32_t *comp_seed,
                      const int32_t *comp_offset, int32_t *members_out);
int pmx_density_destroy(pmx_density *d);

/*
 * What a score is made of, for a list of ligands (a ranked screen's hits): per conformer c < C the float64 maximum over the leaves
 * of the reference's tree (`scores` inside GraphMatcher._run_average, graph_match.py:103-109 - their mean is what pmx_score_f64
 * returns, bit for bit the same values) and the key of the leaf that reaches it (ClusterMatchTree.key, tree.py:129-137): per
 * tree level the model cluster (its index in model.node_clusters) that the level's ligand cluster is matched to, or 0xFF for
 * None. Ties: the FIRST leaf in `root_tree.iteration()` order with that score - the one a strict `>` update keeps; children
 * are in ascending model-cluster order with None last (tree.py:88-101), so this is the lexicographically smallest key with None
 * after every cluster.
 *   ligands_dev[n]        library indices, any order, repeats allowed; an index outside the library is reported PMX_LIGAND_UNSUPPORTED
 *   conf_max_dev          double [n][PMX_MAX_CONFORMERS]: the maxima (0 where no leaf holds the conformer with a score > 0), lanes >= C are 0
 *   match_dev             uint8 [n][PMX_MAX_CONFORMERS][PMX_MAX_LEVELS]: the keys; 0xFF throughout for a conformer whose maximum is 0 and
 *                         for levels >= nl
 *   levels_dev            uint8 [n][PMX_MAX_LEVELS]: the ligand cluster of tree level l (its index in the record's priority-ordered cluster
 *                         list: clusters without a candidate are skipped, at most PMX_MAX_LEVELS, graph_match.py:87-88,124-137); 0xFE for l >= nl
 *   best_conformer_dev    int32 [n]: the smallest c with the largest maximum (-1 for a ligand with a non-zero status)
 *   status_dev            int32 [n]: PMX_LIGAND_* as pmx_score reports it; an unsupported or too large ligand has NaN maxima
 * n <= PMX_EXPLAIN_MAX. The call is stream-ordered like pmx_score (enqueued, no synchronisation) and uses the same workspace of
 * (device, stream). Each listed ligand's tables are built as pmx_score builds them and its tree is walked to its end by one
 * wavefront (pmx_explain.hip): no pass budget, no task queue - the call costs about its largest tree.
 *
 * Constrained matching (pmx_explain_constrained): the same answers over the leaves that QUALIFY under a constraint. A constraint is up
 * to PMX_MAX_REQUIRE_GROUPS require groups - each a non-empty set of model clusters (indices into model.node_clusters) - and one
 * exclude set. A leaf qualifies when its key holds at least one cluster of every require group and no cluster of the exclude set (a
 * group of several clusters says "any cluster that holds this hotspot node"). The tree is the reference's, unchanged: which children
 * exist and when the skip child exists (`nm + mx < 5`, tree.py:98-101) do not depend on the constraint; only the set of leaves that may
 * update a conformer's maximum does. Per conformer the constrained maximum is the maximum over qualifying leaves that hold the
 * conformer with a score > 0 (0 if there is none, keys 0xFF), the key that of the first qualifying leaf in iteration order that
 * reaches it - the rule above. A constrained maximum is never above the unconstrained one. Outputs, limits, statuses, stream ordering
 * and workspace use are pmx_explain's; pmx_explain is this call without a constraint (constraint = NULL).
 *   PMX_ERR_INVALID       n_require outside 0 .. PMX_MAX_REQUIRE_GROUPS; an empty group among the first n_require; a bit at or above the
 *                         model's cluster count
 * A constraint that no leaf can satisfy (a cluster required alone and excluded, say) is no error: status 0, maxima 0, keys 0xFF, best
 * conformer 0.
 */
#define PMX_EXPLAIN_MAX 65536
int pmx_explain(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const uint64_t *ligands_dev, uint32_t n,
                double *conf_max_dev, uint8_t *match_dev, uint8_t *levels_dev, int32_t *best_conformer_dev, int32_t *status_dev, void *stream);

#define PMX_MAX_REQUIRE_GROUPS 8
typedef struct {
    int32_t n_require;                           /* 0 .. PMX_MAX_REQUIRE_GROUPS */
    uint64_t require[PMX_MAX_REQUIRE_GROUPS][2]; /* bit (a % 64) of word a / 64: model cluster a */
    uint64_t exclude[2];
} pmx_match_constraint; /* host struct, copied by the call; NULL = no constraint */

int pmx_explain_constrained(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES],
                            const pmx_match_constraint *constraint, const uint64_t *ligands_dev, uint32_t n, double *conf_max_dev,
                            uint8_t *match_dev, uint8_t *levels_dev, int32_t *best_conformer_dev, int32_t *status_dev, void *stream);

/*
 * The other good binding modes: per listed ligand, per conformer c and per mode m < n_modes, the m-th entry of that conformer's ranked
 * leaf list - the leaves of the reference's tree (`root_tree.iteration()`) that hold c with a score > 0 (and qualify, when a constraint
 * is given), by descending score, equal scores in iteration order (the rule that makes pmx_explain's key "the first leaf"). Values are
 * the float64 leaf totals as the product walker sums them, so mode 0 is bit for bit pmx_explain (constraint = NULL) or
 * pmx_explain_constrained: maxima, keys, levels, best conformer and status.
 *   mode_max_dev          double [n][n_modes][PMX_MAX_CONFORMERS]: the totals, non-increasing in m; 0 for entries beyond the number of such
 *                         leaves and for lanes >= C
 *   mode_match_dev        uint8 [n][n_modes][PMX_MAX_CONFORMERS][PMX_MAX_LEVELS]: their keys in match_dev's format; 0xFF throughout where the
 *                         value is 0
 *   levels_dev, status_dev  as pmx_explain's
 *   best_conformer_dev    defined on mode 0: the smallest c with the largest mode_max[.][0][c] (-1 for a ligand with a non-zero status)
 * A ligand with a non-zero status has NaN in every mode. 1 <= n_modes <= PMX_MAX_MODES and n * n_modes <= PMX_EXPLAIN_MAX, otherwise
 * PMX_ERR_INVALID; the constraint is checked as pmx_explain_constrained checks it; n = 0 succeeds. Statuses, stream ordering and
 * workspace use are pmx_explain's, its slice, large-slice and arena passes included. One wavefront walks a ligand's tree once for all
 * modes (pmx_explain.hip: the one walker, of which pmx_explain is n_modes = 1): a subtree is left out only when no leaf in it can enter any conformer's list, so the call
 * costs more than pmx_explain the further the n_modes-th value lies below the maximum. There is no ranking of modes across conformers: a
 * leaf holds a subset of the conformers, and the reference defines none.
 */
#define PMX_MAX_MODES 8
int pmx_explain_modes(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES],
                      const pmx_match_constraint *constraint /* NULL = none */, int n_modes, const uint64_t *ligands_dev, uint32_t n,
                      double *mode_max_dev, uint8_t *mode_match_dev, uint8_t *levels_dev, int32_t *best_conformer_dev, int32_t *status_dev,
                      void *stream);

/*
 * Which ligand nodes carry a leaf's total: row i takes library ligand ligands_dev[i], conformer conformer_dev[i] and a key key_dev[i] -
 * per tree level a model cluster or 0xFF for None, the format of pmx_explain's match_dev rows - and answers with the entries the
 * reference's tree adds up for that leaf, term by term. All values are for that conformer c; lines of match_utils.py, graph_match.py, tree.py.
 *   levels[l]      the ligand cluster behind tree level l, as pmx_explain reports it (0xFE for l >= nl).
 *   match list     of a matched level l (k[l] != 0xFF; q = levels[l], a = k[l]): the nodes u of cluster q, in record order, whose type mask shares
 *                  a type with at least one node of model cluster a (graph_match.py:139-172).
 *   term(u, v)     likelihood * normalize_coeff * score_coeff of match_utils.py:29-69, in the reference's float32 operations;
 *   fail(u, v)     num_pass < num_match * 0.5 (:56-61).
 *   entry[l][l]    the float32 sum of term over itertools.combinations of level l's list, in that order (:87-120; no majority test).
 *   entry[l1][l2]  l1 < l2, both matched: the float32 sum of term over itertools.product of the two lists; fails[l1][l2] the number of
 *                  failing node pairs. The entry is -1 (no match) when the cluster-distance prefilter of graph_match.py:263-268 fails (it
 *                  fails only if it fails for EVERY conformer of the ligand) or when fails > n1 * n2 * 0.5; otherwise the sum.
 *   valid          c < C, every k[l] != 0xFF is a candidate of level l, and every off-diagonal entry between matched levels is > 0 (tree.py:81).
 *   total          the float64 sum in the product walker's order: per matched level, shallowest first,
 *                  (running + self) + (pair entries with the matched ancestors, shallowest first).
 *   node[u]        float64: half of every term(u, v) / term(v, u) that enters an entry above, each weighted by its entry's
 *                  (float32 sum) / (float64 sum of the same terms) - 1 to within float32 rounding - so that sum_u node[u] = sum of the entries =
 *                  total to float64 rounding. 0 for nodes of unmatched clusters, of clusters beyond the PMX_MAX_LEVELS levels, or outside
 *                  their cluster's match list.
 * Outputs, per row:
 *   total_dev     double [n]                                     NaN when the row is not valid
 *   node_dev      double [n][PMX_MAX_LIGAND_NODES]               NaN throughout when the row is not valid
 *   entry_dev     float  [n][PMX_MAX_LEVELS][PMX_MAX_LEVELS]     upper triangle and diagonal; 0 elsewhere and for unmatched levels, -1 as defined
 *                                                                above. Written for an invalid row too (the answer to "why not this mode"); a
 *                                                                match that is not a candidate of its level counts as None there, and a row
 *                                                                whose conformer is not one of the ligand's has no entries (all 0).
 *   fails_dev     uint16 [n][PMX_MAX_LEVELS][PMX_MAX_LEVELS]     counted in full, also where the entry is -1; 0 on the diagonal
 *   levels_dev    uint8  [n][PMX_MAX_LEVELS]
 *   status_dev    int32  [n]  PMX_LIGAND_OK; PMX_LIGAND_UNSUPPORTED for an index outside the library, a header-only record or a ligand
 *                             pmx_score reports unsupported; PMX_LIGAND_KEY_INVALID for a row that is not valid
 * A key of all 0xFF, or a ligand without levels, is valid with total 0. n <= PMX_EXPLAIN_MAX; n = 0 succeeds. The call is stream-ordered
 * like pmx_explain (enqueued, no synchronisation). One wavefront per row (pmx_rows.hip); no score table, no tabulated pair function,
 * no table arena: any weights, and no dependence on PMX_TAILS_RATIO. The same call gives the same bits on every run.
 */
int pmx_attribute(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const uint64_t *ligands_dev,
                  const int32_t *conformer_dev, const uint8_t *key_dev /* [n][PMX_MAX_LEVELS] */, uint32_t n, double *total_dev, double *node_dev,
                  float *entry_dev, uint16_t *fails_dev, uint8_t *levels_dev, int32_t *status_dev, void *stream);

/*
 * Where a binding mode sits in the pocket: row i takes library ligand ligands_dev[i], conformer c = conformer_dev[i] and a key key_dev[i],
 * in the format of pmx_attribute's rows, and answers with the rigid motion that brings the matched ligand nodes onto the pharmacophore
 * points of the model nodes they are matched to. The reference has no counterpart (it scores distances only); float64 throughout.
 *   pairs      for every matched level l (k[l] != 0xFF; q = levels[l], a = k[l]) and every node u of q in the level's match list (as
 *              pmx_attribute defines it, graph_match.py:139-172): every model node m of cluster a whose type is in u's type mask forms a
 *              pair (u, m) of weight w = weights[node_type[m]]; pairs with w <= 0 are left out. x_u is u's float32 position for
 *              conformer c, widened; y_m = node_center_dev[m], the model node's `center`.
 *   R, t       the proper rotation and the translation that minimise sum_pairs w |R x_u + t - y_m|^2: W = sum w, weighted centroids xbar
 *              and ybar, S = sum w (x_u - xbar)(y_m - ybar)^T, Horn's symmetric 4x4 matrix N of S, its eigenvalues by cyclic Jacobi, the
 *              quaternion q of the largest (the lowest index on equal eigenvalues: N = 0 gives q = (1, 0, 0, 0), R = I), R from q,
 *              t = ybar - R xbar. Never a reflection: a mirrored ligand gets the best proper rotation and a residual. With one fitted
 *              node S is taken as 0: R = I exactly and t = ybar - xbar.
 *   fit[0]     W
 *   fit[1]     sse = sum_pairs w |R x_u + t - y_m|^2, summed from the posed points
 *   fit[2]     rmsd = sqrt(sse / W)
 *   fit[3]     rmsd_nodes = sqrt(sum_u W_u |R x_u + t - ybar_u|^2 / W), W_u and ybar_u node u's weight sum and weighted target centroid
 *              (sse = rmsd_nodes^2 W + sum_u sum_m w |y_m - ybar_u|^2: several targets per node add a constant the fit cannot change)
 *   fit[4]     E0 = sum_pairs w (|x_u - xbar|^2 + |y_m - ybar|^2)
 *   fit[5]     gap = lambda_1 - lambda_2 of N: the rotation is unique only where gap / E0 is not tiny (fitted nodes in one point or on a
 *              line leave a rotation free); the caller decides
 *   fit[6, 7]  0
 * Outputs, per row:
 *   rot_dev     double [n][9]  R, row-major          trans_dev  double [n][3]  t          fit_dev  double [n][8]
 *   node_dev    double [n][PMX_MAX_LIGAND_NODES]  |R x_u + t - ybar_u| of a fitted node (one with a pair); -1 for every other node of the
 *                                                 record and for the lanes beyond it
 *   count_dev   int32  [n][2]  {fitted nodes, pairs}
 *   levels_dev  uint8  [n][PMX_MAX_LEVELS]  as pmx_attribute writes it
 *   status_dev  int32  [n]  PMX_LIGAND_OK; PMX_LIGAND_UNSUPPORTED as pmx_attribute reports it; PMX_LIGAND_KEY_INVALID when c is not a
 *                           conformer of the ligand or some k[l] != 0xFF is not a candidate of level l. The key need not be a leaf of
 *                           the tree: no score is computed, so "what would this mode look like" is allowed.
 * A row that is not OK has NaN in rot, trans, fit and node, and counts of 0. A valid row without pairs (a key of all 0xFF, a ligand without
 * levels, W = 0) has R = I, t = 0 and all fit values 0. n <= PMX_EXPLAIN_MAX; n = 0 succeeds; a NULL node_center_dev with n > 0 is
 * PMX_ERR_INVALID. Stream-ordered like pmx_attribute (enqueued, no synchronisation). One wavefront per row (pmx_rows.hip), fixed-order
 * sums, no floating-point atomic: the same call gives the same bits on every run.
 */
int pmx_align(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES],
              const double *node_center_dev /* [n_nodes][3], model node m's `center` */,
              const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint8_t *key_dev /* [n][PMX_MAX_LEVELS] */, uint32_t n,
              double *rot_dev /* [n][9] row-major R */, double *trans_dev /* [n][3] t */, double *fit_dev /* [n][8] */,
              double *node_dev /* [n][PMX_MAX_LIGAND_NODES] */, int32_t *count_dev /* [n][2] */,
              uint8_t *levels_dev /* [n][PMX_MAX_LEVELS] */, int32_t *status_dev, void *stream);

/*
 * Which model nodes - the hotspots of the pocket - carry a leaf's total: rows (ligand, conformer c, key) exactly as pmx_attribute takes them,
 * and the same leaf. pmx_attribute splits every term(u, v) between the two ligand nodes; the same term is a sum over model node pairs
 * (match_utils.py:29-69), and this call splits it among those. All values are for the row's conformer c.
 *   node pair      (u, v) that enters an entry of pmx_attribute: itertools.combinations of one matched level's match list, or
 *                  itertools.product of two matched levels' lists; u is the earlier node in record order.
 *   inner term     (m, m') for m in u's node subset (the model nodes of u's level's match whose type is in u's type mask) and m' in v's:
 *                  the float32 addend g = (w_m w_m' / std) expf(-0.5 z^2), z = (d(u, v) - mean) / std of the model edge (m, m'), formed
 *                  as match_utils.py:50-69 forms it; it passes when |z| < 2 (:56-60).
 *   G(u, v)        the float64 sum of the pair's g in the order of itertools.product(u's subset, v's subset), both ascending.
 *   term(u, v), scale[e]   pmx_attribute's: the float32 term, and entry / (float64 sum of the entry's terms) of the pair's entry e.
 *   hotspot[m]     float64: the sum of 1/2 (g / G(u, v)) term(u, v) scale[e] over every inner term of every node pair in which m is one
 *                  of the two sides; a term (m, m) gives both halves to m; a pair with G = 0 gives nothing. Summed per node pair, pairs
 *                  in ascending (u, v), per pair the side of u first, per side in ascending order of the other model node. 0 for
 *                  m >= n_nodes and for nodes in no term, so sum_m hotspot[m] = sum of the entries = total to float64 rounding.
 *   terms[m], pass[m]   the inner terms, and the passing ones, counted once for each of their sides that is m.
 *   fingerprint    bit (m % 64) of word m / 64 is set iff terms[m] > 0 and 2 pass[m] >= terms[m]: the majority rule of
 *                  match_utils.py:56-61 read per hotspot - the ligand puts most of what it puts near m at a distance the model expects.
 * Outputs, per row:
 *   total_dev        double [n]                            pmx_attribute's total, bit for bit; NaN when the row is not valid
 *   hotspot_dev      double [n][PMX_MAX_MODEL_NODES]       NaN throughout when the row is not valid
 *   terms_dev        uint32 [n][PMX_MAX_MODEL_NODES]       0 throughout when the row is not valid
 *   pass_dev         uint32 [n][PMX_MAX_MODEL_NODES]       0 throughout when the row is not valid
 *   fingerprint_dev  uint64 [n][PMX_FINGERPRINT_WORDS]     0 when the row is not valid
 *   levels_dev, status_dev   as pmx_attribute writes them, with its validity rule: a key that is no leaf for c gives PMX_LIGAND_KEY_INVALID
 * A key of all 0xFF, or a ligand without levels, is valid with total 0 and everything else 0. n <= PMX_EXPLAIN_MAX; n = 0 succeeds. The call
 * is stream-ordered like pmx_attribute (enqueued, no synchronisation). One wavefront per row (pmx_rows.hip): pmx_attribute's steps, then a
 * lane per model node; fixed-order sums, no floating-point atomic: the same call gives the same bits on every run.
 */
#define PMX_FINGERPRINT_WORDS (PMX_MAX_MODEL_NODES / 64) /* 4 */
int pmx_hotspots(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const uint64_t *ligands_dev,
                 const int32_t *conformer_dev, const uint8_t *key_dev /* [n][PMX_MAX_LEVELS] */, uint32_t n, double *total_dev,
                 double *hotspot_dev /* [n][PMX_MAX_MODEL_NODES] */, uint32_t *terms_dev /* [n][PMX_MAX_MODEL_NODES] */,
                 uint32_t *pass_dev /* [n][PMX_MAX_MODEL_NODES] */, uint64_t *fingerprint_dev /* [n][PMX_FINGERPRINT_WORDS] */,
                 uint8_t *levels_dev /* [n][PMX_MAX_LEVELS] */, int32_t *status_dev, void *stream);

/*
 * Fingerprints compared: a_dev [na][PMX_FINGERPRINT_WORDS] against b_dev [nb][PMX_FINGERPRINT_WORDS] (rows of pmx_hotspots'
 * fingerprint_dev, or any bit sets of that size), out_dev [na][nb] float.
 *   sim(x, y) = (float)popcount(x & y) / (float)popcount(x | y), one float32 division; 1.0f when both are empty.
 * na, nb <= PMX_EXPLAIN_MAX (otherwise PMX_ERR_INVALID); na = 0 or nb = 0 succeeds and writes nothing; a_dev == b_dev is allowed. The
 * pointers are memory of `device`. Stream-ordered, no synchronisation.
 */
int pmx_fingerprint_tanimoto(const uint64_t *a_dev, uint32_t na, const uint64_t *b_dev, uint32_t nb, float *out_dev /* [na][nb] */, int device, void *stream);

/*
 * Sphere exclusion in row order (the rows are the caller's ranking, best first): row i joins the FIRST earlier leader l with
 * sim(fp[i], fp[l]) >= threshold, compared in float32 - leader_of[i] = l; otherwise it becomes a leader, leader_of[i] = i. Once max_leaders
 * leaders exist a row that joins none gets UINT32_MAX. Row 0 is always a leader when n > 0. Similarity is not transitive and the rule does
 * not pretend it is: a row similar to a member of a leader's cluster but not to the leader does not join it.
 *   leader_of_dev  uint32 [n]            leaders_dev  uint32 [max_leaders]: the leaders' rows, ascending; the first *n_leaders_dev are written
 *   n_leaders_dev  uint32 [1]
 * PMX_ERR_INVALID: threshold outside (0, 1]; max_leaders 0 or above PMX_MAX_LEADERS; n > PMX_EXPLAIN_MAX. n = 0 succeeds with
 * *n_leaders_dev = 0. The result is defined by the rule alone. One work-group with the leaders' fingerprints in LDS
 * (pmx_fingerprint.hip). Stream-ordered, no synchronisation.
 */
#define PMX_MAX_LEADERS 2048
int pmx_fingerprint_leaders(const uint64_t *fp_dev /* [n][PMX_FINGERPRINT_WORDS] */, uint32_t n, float threshold, uint32_t max_leaders,
                            uint32_t *leader_of_dev /* [n] */, uint32_t *leaders_dev /* [max_leaders] */, uint32_t *n_leaders_dev /* [1] */,
                            int device, void *stream);

/*
 * A ligand described by its own pharmacophore (pmx_ligand_fp.hip): per ligand of a resident library a two-point pharmacophore fingerprint -
 * which unordered pairs of feature types it holds at which distance - in the 256-bit format pmx_fingerprint_tanimoto and
 * pmx_fingerprint_leaders take, and a census of its types. The reference has no counterpart (it describes a ligand only against a pocket);
 * the specification is this comment, and tests/ligand_fp_ref.py restates it in NumPy. Integer results: no tolerance anywhere.
 * For ligand first + i, whose record has n nodes, C conformers and type masks tm[u] (pharmaconet_amd/library.py):
 *   node pairs   every u < v in record order; clusters play no part
 *   d2           for conformer c, in float32: dx, dy, dz the float32 differences of the record's coordinates, d2 = (dx*dx + dy*dy) + dz*dz,
 *                every operation rounded to float32, no fused multiply-add, no square root
 *   bin          the number of entries of E2 = {4, 9, 16, 25, 36, 56.25, 81, 144} - the squares of 2, 3, 4, 5, 6, 7.5, 9 and 12 Angstrom,
 *                all exact in float32 - with d2 >= E2[k]: 0 .. 8; a NaN d2 gives bin 0
 *   type pair    for every type a set in tm[u] and b set in tm[v]: lo = min(a, b), hi = max(a, b), p = lo * (15 - lo) / 2 + (hi - lo): 0 .. 27
 *   bit          j = p * PMX_LFP_BINS + bin (0 .. 251) is set: bit j % 64 of word j / 64. Bits 252 .. 255 are always 0
 *   conformers   conformer_dev == NULL or conformer_dev[i] == -1: a bit is set when any conformer c < C sets it - the union, what the
 *                ligand can present; conformer_dev[i] = c >= 0: that conformer alone - a hit as posed (pmx_explain's best_conformer, say)
 * Outputs, per ligand:
 *   fingerprint_dev  uint64 [count][PMX_FINGERPRINT_WORDS]
 *   type_count_dev   uint8 [count][8] or NULL: for t = 0 .. 6 the number of nodes with type t in their mask; entry [7] is n
 *   status_dev       int32 [count] or NULL: PMX_LIGAND_OK; PMX_LIGAND_UNSUPPORTED for a record pmx_score reports so by its header (more than
 *                    PMX_MAX_LIGAND_NODES nodes or PMX_MAX_LIGAND_CLUSTERS clusters, no conformer or more than PMX_MAX_CONFORMERS - header-only
 *                    records included): fingerprint and counts are 0; PMX_LIGAND_KEY_INVALID where conformer_dev[i] < -1 or >= C: the
 *                    fingerprint is 0, the counts are still written. A supported record with n < 2 is OK with an empty fingerprint.
 * first + count > n_ligands is PMX_ERR_INVALID; count = 0 succeeds. Stream-ordered like pmx_score (enqueued, no synchronisation), no work
 * buffer. One wavefront per ligand; OR is order-free, so the same bits come out however the work is laid out.
 */
#define PMX_LFP_BINS 9
int pmx_library_fingerprints(const pmx_library *lib, uint64_t first, uint64_t count, const int32_t *conformer_dev /* [count] or NULL */,
                             uint64_t *fingerprint_dev /* [count][PMX_FINGERPRINT_WORDS] */, uint8_t *type_count_dev /* [count][8] or NULL */,
                             int32_t *status_dev /* [count] or NULL */, void *stream);

/*
 * Similarity search (pmx_ligand_fp.hip): nq query fingerprints against a list of n, of any length - pmx_fingerprint_tanimoto stops at
 * 65536 rows a side, a library has 10^6 or more.
 *   out_dev[q][i]   float32 [nq][out_stride]: sim(query[q], fp[i]) exactly as pmx_fingerprint_tanimoto defines it - one float32 division,
 *                   1.0f when both sets are empty. The layout pmx_topk (a row) and pmx_enrichment (col_stride = out_stride) take as it is
 *   fused_dev[i]    float32 [n] or NULL: the maximum over q - MAX fusion, the usual rule for several reference ligands
 * n < 2^31, 1 <= nq <= PMX_SEARCH_MAX_QUERIES and out_stride >= n, otherwise PMX_ERR_INVALID; n = 0 succeeds and writes nothing. The
 * pointers are memory of `device`. Each library fingerprint is read once for all queries (a thread per fingerprint). Stream-ordered, no
 * synchronisation.
 */
#define PMX_SEARCH_MAX_QUERIES 64
int pmx_fingerprint_search(const uint64_t *query_dev /* [nq][PMX_FINGERPRINT_WORDS] */, uint32_t nq, const uint64_t *fp_dev /* [n][PMX_FINGERPRINT_WORDS] */,
                           uint64_t n, float *out_dev /* [nq][out_stride] */, uint64_t out_stride, float *fused_dev /* [n] or NULL */, int device, void *stream);

/*
 * Excluded volumes (pmx_pocket.hip): does a posed hit fit where pmx_align puts it? Every row of a call is a set of points under a rigid
 * motion, checked against the atoms of the pocket: how deep the worst pair penetrates, how much overlaps in all, how many points clash and
 * touch, and which residues are touched. The reference has no counterpart (it scores distances between pharmacophore points only); the
 * specification is this comment, and tests/clash_ref.py restates it in NumPy.
 *
 * The pocket: pmx_pocket_create copies n <= PMX_POCKET_MAX_ATOMS atoms - float32 positions xyz[n][3] in the model's frame, radii radius[n]
 * (the caller's: pharmaconet_amd/pocket.py uses Bondi's) and a group per atom (group[n], or NULL for "no group": 0xFFFF throughout) - to
 * `device`. A group below 256 is a residue's bit of contact_fp; any other value is an atom outside the 256. n = 0 is allowed: a pocket
 * without atoms. The copy is finished when the call returns. pmx_pocket_destroy frees it (NULL is allowed).
 *
 * The points of row i, one of two sources per call (both, or neither, is PMX_ERR_INVALID):
 *   node mode    lib given, point_off_dev, points_dev and point_radius_dev NULL: the n_i nodes of library ligand ligands_dev[i] at conformer
 *                conformer_dev[i], in record order, the record's float32 coordinates, each of radius point_radius
 *   point mode   lib NULL: points_dev[point_off_dev[i] .. point_off_dev[i + 1]), float32 [.][3] - a whole molecule's atoms, say - with
 *                radii point_radius_dev[.], or point_radius each where that pointer is NULL; ligands_dev and conformer_dev are not read
 * Arithmetic, float64 with every operation rounded (no fused multiply-add), R = rot_dev[i] row-major, t = trans_dev[i], x widened:
 *   posed point  p_k = ((R[k][0] x_0 + R[k][1] x_1) + R[k][2] x_2) + t_k
 *   pair         point p of radius r_p, atom a at float32 y with radius r_a: dx, dy, dz = p - y; d = sqrt((dx dx + dy dy) + dz dz);
 *                s = ((double)r_a + (double)r_p) - (double)tolerance; pen = s - d
 *                the pair clashes iff pen > 0; it touches iff d < (double)contact
 * Outputs, per row:
 *   summary_dev     double [n][4]  [0] the largest pen over all pairs - negative when nothing clashes (the clearance), -inf with no point
 *                                  or no atom; [1] the overlap: the sum of pen^2 over the clashing pairs; [2], [3] 0
 *   count_dev       int32 [n][6]   [0] points; [1] points with a clashing pair; [2] clashing pairs; [3] points that touch some atom;
 *                                  [4], [5] the point and the atom of summary[0] - the lowest point, then the lowest atom, among equals -
 *                                  and -1 where there is no pair
 *   point_pen_dev, point_atom_dev  per point its largest pen and the lowest-index atom that attains it (-inf and -1 for a pocket without
 *                                  atoms). Node mode: double / int32 [n][PMX_MAX_LIGAND_NODES], NaN / -1 beyond the record's nodes; point
 *                                  mode: [point_off_dev[n]], the layout of the points
 *   contact_fp_dev  uint64 [n][PMX_FINGERPRINT_WORDS] or NULL: bit g % 64 of word g / 64 is set iff some atom of group g < 256 touches
 *                                  some point of the row - the format pmx_fingerprint_tanimoto and pmx_fingerprint_leaders take
 *   status_dev      int32 [n]      PMX_LIGAND_OK; node mode: PMX_LIGAND_UNSUPPORTED for an index outside the library and for a record that
 *                                  pmx_score reports so by its header (header-only records included), PMX_LIGAND_KEY_INVALID when
 *                                  conformer_dev[i] is not a conformer of the ligand (-1 is none); both modes: PMX_LIGAND_KEY_INVALID when
 *                                  any of the row's 12 motion values is not finite - what pmx_align hands out for its own rows that are
 *                                  not OK, so that such a row passes through with a status
 * A row that is not OK has NaN in all of summary, counts of 0 with [4] = [5] = -1, NaN / -1 for every point it has room for, and an empty
 * set. The overlap is summed per point in atom order, a lane's points in ascending order, the 64 lanes (point % 64) by a fixed butterfly:
 * fixed-order sums, no floating-point atomic, the same bits on every run and for a row wherever it stands in a call.
 * n <= PMX_EXPLAIN_MAX (otherwise PMX_ERR_INVALID); n = 0 succeeds and writes nothing. With n > 0 only contact_fp_dev may be NULL among the
 * outputs; point_radius, tolerance and contact must be finite; in node mode the library is on the pocket's device. The pointers are memory of
 * that device. Stream-ordered like pmx_align (enqueued, no synchronisation), no work buffer. One wavefront per row, a lane per point.
 */
#define PMX_POCKET_MAX_ATOMS 65536
typedef struct pmx_pocket pmx_pocket;
int pmx_pocket_create(const float *xyz /* [n][3] */, const float *radius /* [n] */, const uint16_t *group /* [n] or NULL */, uint32_t n, int device,
                      pmx_pocket **out);
int pmx_pocket_destroy(pmx_pocket *pocket);
int pmx_pose_clash(const pmx_pocket *pocket, const pmx_library *lib /* NULL in point mode */, const uint64_t *ligands_dev, const int32_t *conformer_dev /* node mode: [n] each */,
                   const uint64_t *point_off_dev /* [n + 1] */, const float *points_dev /* [.][3] */, const float *point_radius_dev /* [.] or NULL */,
                   const double *rot_dev /* [n][9] */, const double *trans_dev /* [n][3] */, uint32_t n, float point_radius, float tolerance, float contact,
                   double *summary_dev /* [n][4] */, int32_t *count_dev /* [n][6] */, double *point_pen_dev, int32_t *point_atom_dev,
                   uint64_t *contact_fp_dev /* [n][PMX_FINGERPRINT_WORDS] or NULL */, int32_t *status_dev, void *stream);

/*
 * Restrained rigid-body clash relief (pmx_refine.hip): a pose whose least-squares fit grazes a side chain is moved out of it, one that runs
 * through the backbone stays rejected. Per row a bounded, deterministic Levenberg-Marquardt minimisation over the six rigid degrees of
 * freedom of E = Ec + restraint Er: the overlap pmx_pose_clash defines, plus a harmonic restraint that holds anchors near where the start
 * motion put them. The reference has no counterpart; the specification is this comment, and tests/refine_ref.py restates it in NumPy.
 *
 * Points: a row's points, their radii, node mode and point mode, and the status rules are pmx_pose_clash's (a start motion that is not
 * finite: PMX_LIGAND_KEY_INVALID; a record that is not supported: PMX_LIGAND_UNSUPPORTED).
 * Anchors, what the restraint holds: with anchor_off_dev NULL the row's own points, each of weight 1 (anchors_dev, anchor_target_dev and
 * anchor_weight_dev are then NULL too). Otherwise anchors_dev[anchor_off_dev[i] .. anchor_off_dev[i + 1]), float32 [.][3] in the
 * conformer's frame, with weights anchor_weight_dev[.] (float64; 1 each where that pointer is NULL; a weight that is negative or not finite
 * gives the row PMX_LIGAND_KEY_INVALID) and targets anchor_target_dev[.][3] (float64, the pocket's frame; where that pointer is NULL an
 * anchor's target is its own position under the row's start motion, by the posed-point formula: "stay where the fit put you").
 *
 * Energy at a motion (R, t). Posed points p (and posed anchors q) and the pairs' d and pen by the operations of the pmx_pose_clash comment:
 * float64, every operation rounded, no fused multiply-add.
 *   Ec = the sum of pen^2 over the pairs with pen > 0, in pmx_pose_clash's order (per point in atom order, a lane's points ascending, the
 *        fixed butterfly over the 64 lanes)
 *   Er = the sum over the anchors of w ((e_0 e_0 + e_1 e_1) + e_2 e_2), e = q - b (a lane's anchors, anchor % 64, ascending; the butterfly)
 *   E  = Ec + restraint * Er
 * Normal equations at (R, t). c = the sum of the posed points (summed like Er) / the number of points, 0 for a row without points. A small
 * motion is delta p = omega x (p - c) + tau. A clashing pair with d > 0 and nhat = (dx, dy, dz) / d has the residual pen and the Jacobian row
 * -v, v = [(p - c) x nhat, nhat]; a pair with d == 0 counts in Ec only. An anchor at q has the three residuals sqrt(restraint w) (q - b) with
 * rows sqrt(restraint w) [-[q - c]_x, I]: in closed form, with r = q - c and k = restraint * w, the blocks k (|r|^2 I - r r^T), k [r]_x, k I
 * of H and k [r x e, e] of g. H = sum J^T J (6 x 6, 21 values), g = sum J^T r; per lane the pairs' terms in (point, atom) order, then the
 * anchors', and the butterfly.
 * Iteration:
 *   1. evaluate at the start motion
 *   2. no pair clashes: stop, reason 0 - the outputs are the input motion bit for bit
 *   3. otherwise lambda = 1e-3, and while iterations < max_iter:
 *        solve (H + lambda diag(H_ii + 1e-9)) delta = -g by Cholesky; omega = delta[0 .. 3), tau = delta[3 .. 6)
 *        Rd = I + (sin th / th) K + (2 sin^2(th / 2) / th^2) K^2, K = [omega]_x, th = |omega| (the identity at th = 0)
 *        trial: R' = Rd R, t' = Rd (t - c) + c + tau; evaluate there; ++iterations
 *        E' < E: accept, lambda = max(lambda / 4, 1e-9); if E - E' <= ftol * E: stop, reason 1
 *        otherwise: lambda *= 8; if lambda > 1e8: stop, reason 3
 *      (a pivot of the Cholesky that is not positive, or a delta that is not finite, is a rejected trial: it counts as an iteration
 *      without an evaluation)
 *   4. running out of max_iter: reason 2. 0 <= max_iter <= PMX_REFINE_MAX_ITER; max_iter = 0 evaluates and returns the start.
 * The loop is bounded by max_iter evaluations whatever the data; no other loop depends on convergence.
 * Outputs, per row:
 *   rot_out_dev, trans_out_dev   double [n][9], [n][3]: the last accepted motion
 *   energy_dev   double [n][8]   Ec at the start, Er at the start, Ec final, Er final, the anchor rmsd sqrt(Er / sum w) (0 without weight),
 *                                the net rotation angle from the start in rad (0 when no step was accepted), |c_final - c_start|, the
 *                                final lambda
 *   count_dev    int32 [n][4]    iterations, accepted steps, stop reason, clashing pairs at the final motion
 *   status_dev   int32 [n]       PMX_LIGAND_*
 * A row that is not OK has NaN motions and energies, counts of 0 and a stop reason of -1.
 * Cross-checks. Every evaluation poses the points from the stored (R, t) by the formula above, so bit for bit: Ec at the start is
 * pmx_pose_clash's overlap at the input motion; Ec final and count[3] are pmx_pose_clash's overlap and pair count at rot_out / trans_out.
 * n <= PMX_EXPLAIN_MAX (otherwise PMX_ERR_INVALID); n = 0 succeeds and writes nothing. restraint >= 0 and ftol >= 0, both finite;
 * point_radius and tolerance finite; one source of points per call; in node mode the library is on the pocket's device; no output may be
 * NULL: otherwise PMX_ERR_INVALID. The pointers are memory of that device. Stream-ordered (enqueued, no synchronisation), no work buffer,
 * no floating-point atomic: the same bits on every run, and for a row wherever it stands in a call. One wavefront per row.
 */
#define PMX_REFINE_MAX_ITER 64
int pmx_pose_refine(const pmx_pocket *pocket, const pmx_library *lib /* NULL in point mode */, const uint64_t *ligands_dev, const int32_t *conformer_dev,
                    const uint64_t *point_off_dev, const float *points_dev, const float *point_radius_dev,
                    const uint64_t *anchor_off_dev /* [n + 1] or NULL */, const float *anchors_dev /* [.][3] */,
                    const double *anchor_target_dev /* [.][3] or NULL */, const double *anchor_weight_dev /* [.] or NULL */,
                    const double *rot_dev, const double *trans_dev, uint32_t n, float point_radius, float tolerance, double restraint, double ftol,
                    int max_iter, double *rot_out_dev /* [n][9] */, double *trans_out_dev /* [n][3] */, double *energy_dev /* [n][8] */,
                    int32_t *count_dev /* [n][4] */, int32_t *status_dev, void *stream);

/*
 * The atom store (pmx_atoms.hip): each ligand's heavy atoms resident next to its record, so that the point-mode rows of pmx_pose_clash and
 * pmx_pose_refine - a whole molecule's atoms - can be made on the device, for any (ligand, conformer), without a host array. A store is the
 * companion of a library: one record per ligand, in the library's order, the coordinates in the record's own frame (what pmx_align's
 * motion applies to). The reference has no counterpart; the specification is this comment, and tests/atoms_ref.py restates it in NumPy.
 *
 * A record (little endian, 16-byte aligned like a ligand record):
 *   u16 n_atoms | u16 n_conf | u32 0
 *   u8  element[n_atoms]          atomic numbers of the heavy atoms (Z > 1), in the molecule's order, each <= 127
 *   pad to 4 bytes
 *   f32 xyz[n_atoms][n_conf][3]   the molecule's atom positions, heavy atoms only, as the perception hands them over
 *   pad to 16 bytes
 * n_atoms <= PMX_MAX_LIGAND_ATOMS, 1 <= n_conf <= PMX_MAX_CONFORMERS. A header-only record - 16 bytes, n_atoms = 0 - means "no atoms
 * kept": a molecule with more heavy atoms than that, with none, or whose ligand record is the unsupported marker.
 * A store is offsets u64[n_ligands + 1] (offsets[0] = 0, bytes) and data; pharmaconet_amd/atoms.py (PackedAtoms) builds and stores it.
 *
 * pmx_atoms_upload copies a host store to `device` and with it radius_of_element[128], the radius of a point by atomic number (the
 * caller's: pharmaconet_amd/pocket.py's Bondi table, so that a gathered radius is the host path's bit for bit). It checks on the host, before
 * anything is copied: offsets rising in multiples of 16, every header within the limits and consistent with its record's size, every
 * element <= 127 - otherwise PMX_ERR_INVALID, so that no kernel has to doubt a record. The copy is finished when the call returns.
 * pmx_atoms_info_get: n_ligands, n_bytes, max_atoms (the largest n_atoms) and n_empty (header-only records). pmx_atoms_destroy frees the
 * copy (NULL is allowed).
 *
 * pmx_atoms_gather: row i < n is the heavy atoms of ligand ligands_dev[i] at conformer conformer_dev[i], in record order:
 *   point_off_dev     uint64 [n + 1]  point_off[0] = 0; row i's points are [point_off[i], point_off[i + 1])
 *   points_dev        float32 [cap_points][3]  the record's float32 coordinates of that conformer, copied
 *   point_radius_dev  float32 [cap_points]     radius_of_element[element]
 *   status_dev        int32 [n]  PMX_LIGAND_OK; PMX_LIGAND_UNSUPPORTED for an index outside the store and for a header-only record (whatever
 *                     the conformer); otherwise PMX_LIGAND_KEY_INVALID for a conformer < 0 or >= the record's n_conf
 * A row that is not OK has no points: point_off[i + 1] == point_off[i]. These are the three point-mode arguments of pmx_pose_clash and
 * pmx_pose_refine; a caller that wants a row without atoms reported as not OK - in point mode an empty row is a valid row with clearance
 * -inf - merges status_dev into theirs (pmx_pose_search_atoms does).
 * n <= PMX_EXPLAIN_MAX and cap_points >= n * max_atoms of the store: otherwise PMX_ERR_INVALID - checked on the host, so that no row can
 * write past the buffers and nothing has to be read back. n = 0 succeeds and writes point_off[0] = 0 only. With n > 0 no pointer may be
 * NULL; the pointers are memory of the store's device. Stream-ordered (enqueued, no synchronisation), no allocation, no work buffer, no
 * atomic: the same bits on every run, and for a row wherever it stands in a call. Three kernels: a size per row, one block's scan of the
 * sizes into point_off_dev, one wavefront per row for the copy.
 */
#define PMX_MAX_LIGAND_ATOMS 256
typedef struct pmx_atoms pmx_atoms;
typedef struct {
    uint64_t n_ligands;
    const uint64_t *offsets; /* [n_ligands + 1], host */
    const uint8_t *data;     /* host */
} pmx_atoms_view;
typedef struct {
    uint64_t n_ligands;
    uint64_t n_bytes;
    int32_t max_atoms;
    int32_t n_empty;
} pmx_atoms_info;
int pmx_atoms_upload(const pmx_atoms_view *view, const float radius_of_element[128], int device, pmx_atoms **out);
int pmx_atoms_info_get(const pmx_atoms *atoms, pmx_atoms_info *info);
int pmx_atoms_destroy(pmx_atoms *atoms);
int pmx_atoms_gather(const pmx_atoms *atoms, const uint64_t *ligands_dev, const int32_t *conformer_dev, uint32_t n, uint64_t cap_points,
                     uint64_t *point_off_dev /* [n + 1] */, float *points_dev /* [cap_points][3] */, float *point_radius_dev /* [cap_points] */,
                     int32_t *status_dev /* [n] */, void *stream);

/*
 * Pose search (pmx_pose_search.hip): which of a hit's conformers, under which of its binding modes, to pose. pmx_explain's single pose -
 * the best conformer under its own key - often grazes a side chain where the second conformer, or the same conformer under its second
 * mode, sits in the cavity. The call takes the output of a pmx_explain_modes call over exactly ligands_dev[n] (with or without a
 * constraint) - mode_max_dev [n][n_modes][PMX_MAX_CONFORMERS], mode_match_dev [n][n_modes][PMX_MAX_CONFORMERS][PMX_MAX_LEVELS] and its
 * status_dev [n] (explain_status_dev) - fits the slots with pmx_align, checks the fits with pmx_pose_clash in node mode, and chooses one
 * slot per hit. The reference has no counterpart; the specification is this comment, and tests/pose_search_ref.py restates it in NumPy.
 *
 * Slot (i, m, c), m < n_modes, c < conf_stride (the conformers searched per hit; a ligand with fewer has zeros there), v = mode_max[i][m][c].
 *   vbest      of hit i: the largest v > 0 over its slots (0 when there is none, or when the hit's explain status is not 0)
 *   row        of a slot: (ligands_dev[i], c, mode_match[i][m][c]) as pmx_align and pmx_pose_clash take rows; model, lib, weights and
 *              node_center_dev are pmx_align's, point_radius, tolerance and contact pmx_pose_clash's
 *   candidate  a slot for which all of these hold: the explain status of hit i is 0; v > 0; pmx_align of the row has status OK and
 *              count[0] >= min_fitted fitted nodes; pmx_pose_clash of the row under that motion has status OK; v >= min_fraction * vbest,
 *              the product formed in float64
 *   dropped    a slot of a hit with explain status 0 and v > 0 for which v >= min_fraction * vbest does not hold, whatever its fit
 *   passes     a candidate whose count of points with a clashing pair (pmx_pose_clash's count[1]) is <= max_clashing
 *   the choice among the passing candidates: the largest v, then the lowest c, then the lowest m. When no candidate passes, among the
 *              candidates: the smallest overlap (pmx_pose_clash's summary[1]), then the largest v, then the lowest c, then the lowest m.
 *              Without a candidate there is no choice.
 * Every comparison is on the float64 bits the two calls produce, or on integers: nothing new is rounded but fraction below.
 * Consequence: where the default pose - the hit's best conformer under mode 0, what pmx_explain poses - passes and has min_fitted fitted
 * nodes, it is the choice: it has the largest v of all slots, the lowest c among those that reach it, and m = 0.
 * Outputs, per hit:
 *   choice_dev  int32 [n][6]   conformer, mode (-1, -1 without a choice), passes 0 / 1, candidates, passing candidates, dropped slots
 *   value_dev   double [n][2]  v of the choice and v / vbest; NaN without a choice
 *   key_dev     uint8 [n][PMX_MAX_LEVELS]  the choice's key; 0xFF throughout without a choice
 *   rot_dev, trans_dev, fit_dev, node_dev, count_dev, levels_dev   what pmx_align writes for the row (ligand, conformer, key) of the
 *               choice, bit for bit; without a choice the row has conformer -1: NaN and counts of 0, as for any pmx_align row that is not OK
 *   summary_dev, clash_count_dev, point_pen_dev, point_atom_dev, contact_fp_dev   what pmx_pose_clash writes for that row under that
 *               motion, bit for bit (without a choice: a row that is not OK)
 *   status_dev  int32 [n]      the hit's explain status. "Nothing to pose" is no error: status 0 with 0 candidates
 *   row_status_dev  int32 [2][n]  the statuses pmx_align ([0][i]) and pmx_pose_clash ([1][i]) give that row: OK with a choice, and
 *               otherwise what says why a hit could not be posed at all (PMX_LIGAND_UNSUPPORTED or PMX_LIGAND_KEY_INVALID)
 * 1 <= n_modes <= PMX_MAX_MODES, 1 <= conf_stride <= PMX_MAX_CONFORMERS, max_clashing >= 0, min_fitted >= 1, min_fraction in [0, 1],
 * point_radius, tolerance and contact finite, n * n_modes * conf_stride <= PMX_EXPLAIN_MAX: otherwise PMX_ERR_INVALID. n = 0 succeeds and
 * writes nothing. With n > 0 no pointer may be NULL; the library is on the pocket's device and the pointers are memory of it.
 * work_dev: at least pmx_pose_search_work_bytes(n, n_modes, conf_stride) bytes of that device, 16-byte aligned, the caller's; its
 * contents mean nothing before or after. The query answers 0 for a shape the call would refuse and grows with each argument.
 * The call allocates nothing and synchronises nothing: stream-ordered like pmx_align, whose workspace of (device, stream) it uses. A
 * kernel writes the slots' rows into the work buffer (a slot that cannot be a candidate by its v alone gets conformer -1 and passes
 * through both calls as PMX_LIGAND_KEY_INVALID), pmx_align and pmx_pose_clash run on them, a second kernel - one wavefront per hit, its
 * lanes over the hit's slots in trips of 64, a lexicographic reduction of fixed shape - chooses, and the two calls run once more on the n
 * chosen rows. No atomic: the same bits on every run, and for a hit wherever it stands in a call.
 */
uint64_t pmx_pose_search_work_bytes(uint32_t n, int n_modes, int conf_stride);
int pmx_pose_search(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const double *node_center_dev,
                    const pmx_pocket *pocket, const uint64_t *ligands_dev, uint32_t n, const double *mode_max_dev, const uint8_t *mode_match_dev,
                    const int32_t *explain_status_dev, int n_modes, int conf_stride, float point_radius, float tolerance, float contact,
                    int max_clashing, int min_fitted, double min_fraction, int32_t *choice_dev /* [n][6] */, double *value_dev /* [n][2] */,
                    uint8_t *key_dev /* [n][PMX_MAX_LEVELS] */, double *rot_dev, double *trans_dev, double *fit_dev, double *node_dev,
                    int32_t *count_dev /* [n][2] */, uint8_t *levels_dev, double *summary_dev, int32_t *clash_count_dev /* [n][6] */,
                    double *point_pen_dev, int32_t *point_atom_dev, uint64_t *contact_fp_dev, int32_t *status_dev,
                    int32_t *row_status_dev /* [2][n] */, void *work_dev, uint64_t work_bytes, void *stream);

/*
 * Pose search at atom level (pmx_pose_search.hip): pmx_pose_search with the clash check made on the ligand's heavy atoms, taken from an
 * atom store (pmx_atoms, above) that is the companion of `lib`. Where the node-level search picks a pose whose pharmacophore nodes are
 * clear, the atoms between them may still run through a side chain; this call chooses on what the next step would check. Nodes are
 * still what pmx_align fits. The rule is pmx_pose_search's word for word, with two changes:
 *   row        of a slot: pmx_align's row as there; the clash check is pmx_pose_clash in point mode on the row pmx_atoms_gather makes of
 *              (ligands_dev[i], c) - the store's coordinates, the store's radii by element - under the fitted motion. point_radius is not
 *              read (every point has its own radius) but must be finite
 *   candidate  additionally: pmx_atoms_gather of the row has status OK. A slot whose gather status is not OK gets that status as its
 *              clash status - in point mode a row without points would pass with clearance -inf
 *   passes, the choice, dropped, vbest: as there, on the atoms' count[1] and summary[1]
 * Consequence: where the default pose - the hit's best conformer under mode 0 - has atoms in the store, passes at atom level and has
 * min_fitted fitted nodes, it is the choice.
 * Outputs, per hit: choice_dev, value_dev, key_dev, status_dev and the pmx_align outputs as pmx_pose_search's. The clash outputs are those
 * of the chosen row in point-mode layout: summary_dev, clash_count_dev, contact_fp_dev as there; point_off_dev uint64 [n + 1] what
 * pmx_atoms_gather writes for the n chosen rows (a hit without a choice has no points); point_pen_dev double and point_atom_dev int32 in
 * that layout, each with room for n * max_atoms of the store.
 *   row_status_dev  int32 [3][n]  the statuses pmx_align ([0][i]), pmx_atoms_gather ([1][i]) and pmx_pose_clash ([2][i]) give the chosen
 *               row; [2][i] is [1][i] where that is not OK. A hit whose atom record is header-only has no choice and [1][i] =
 *               PMX_LIGAND_UNSUPPORTED
 * Limits and errors as pmx_pose_search's; the store is on the library's device. work_dev: at least
 * pmx_pose_search_atoms_work_bytes(n, n_modes, conf_stride, max_atoms) bytes, max_atoms the store's (pmx_atoms_info); the query answers 0
 * for a shape the call would refuse (max_atoms outside 0 .. PMX_MAX_LIGAND_ATOMS included) and grows with each argument. The call allocates
 * nothing and synchronises nothing. Its kernels are pmx_pose_search's two, unchanged, and a status merge; between them pmx_align,
 * pmx_atoms_gather and pmx_pose_clash run on the slots, and once more on the n chosen rows. No atomic: the same bits on every run, and for
 * a hit wherever it stands in a call.
 */
uint64_t pmx_pose_search_atoms_work_bytes(uint32_t n, int n_modes, int conf_stride, int max_atoms);
int pmx_pose_search_atoms(const pmx_model *model, const pmx_library *lib, const pmx_atoms *atoms, const float weights[PMX_NUM_TYPES],
                          const double *node_center_dev, const pmx_pocket *pocket, const uint64_t *ligands_dev, uint32_t n,
                          const double *mode_max_dev, const uint8_t *mode_match_dev, const int32_t *explain_status_dev, int n_modes,
                          int conf_stride, float point_radius, float tolerance, float contact, int max_clashing, int min_fitted,
                          double min_fraction, int32_t *choice_dev /* [n][6] */, double *value_dev /* [n][2] */,
                          uint8_t *key_dev /* [n][PMX_MAX_LEVELS] */, double *rot_dev, double *trans_dev, double *fit_dev, double *node_dev,
                          int32_t *count_dev /* [n][2] */, uint8_t *levels_dev, double *summary_dev, int32_t *clash_count_dev /* [n][6] */,
                          uint64_t *point_off_dev /* [n + 1] */, double *point_pen_dev, int32_t *point_atom_dev, uint64_t *contact_fp_dev,
                          int32_t *status_dev, int32_t *row_status_dev /* [3][n] */, void *work_dev, uint64_t work_bytes, void *stream);

/*
 * Pose fit (pmx_pose_fit.hip): do the ligand's pharmacophore nodes sit on the pocket's hotspots once a pose exists? pmx_align reports a
 * residual over the pairs it was told to fit, pmx_pose_refine moves the ligand and rescores nothing, and the reference's score reads
 * internal distances only - one number for every rigid placement. This call scores the placement: the Gaussian overlap of the posed ligand
 * nodes with the model nodes in the pocket's frame, with the model node's radius as its positional sigma (the reference's own reading of
 * it: an edge's distance_std is sqrt(r1^2 + r2^2), utils/density_map.py:277) and the reference's conventions for a term - weight *
 * exp(-z^2 / 2), passing iff |z| < 2, the majority rule per node (match_utils.py:51-69). The reference has no counterpart; the
 * specification is this comment, and tests/pose_fit_ref.py restates it in NumPy.
 *
 * Row i: library ligand ligands_dev[i] at conformer conformer_dev[i] under R = rot_dev[i] (row-major), t = trans_dev[i]. The points are
 * the record's n_i nodes in record order, exactly as pmx_pose_clash takes them in node mode.
 * Pairs (u, m) of a ligand node u and a model node m, one of two modes per call:
 *   key mode    key_dev given: the pairs of pmx_align for (ligand, conformer, key_dev[i]) - for every matched level, every node u of its
 *               cluster and every model node m of the matched cluster whose type is in u's type mask - from the same row front end
 *   free mode   key_dev NULL: every node u of the record with every model node m whose type is in u's type mask: what the pose touches,
 *               whatever match produced it - and poses that came from elsewhere
 *   In both modes a pair is left out when w = (double)weights[node_type[m]] <= 0, and when s_m = node_sigma_dev[m] is not a finite number > 0.
 * Arithmetic, float64 with every operation rounded (no fused multiply-add), x widened from the record's float32:
 *   posed point  p_u by pmx_pose_clash's formula
 *   pair         e = p_u - y_m, y_m = node_center_dev[m]; d2 = (e_0 e_0 + e_1 e_1) + e_2 e_2; v = s_m s_m; z2 = d2 / v;
 *                the pair passes iff d2 < 4.0 v; g = w exp(-0.5 z2)
 * Per node u with n_u > 0 pairs, its model nodes in ascending m:
 *   node_fit[u]     (the sum of g, in ascending m) / (double)n_u - the reference's mean over a node's matches
 *   W_u             (the sum of w, in ascending m) / (double)n_u - what node_fit[u] is with every pair at z = 0
 *   node_target[u]  the m of the smallest z2, the lowest m among equals; node_z2[u] that z2; node_best[u] the g of that pair
 *   in place        iff 2 pass_u >= n_u, pass_u the node's passing pairs
 *   A node without a pair, and the lanes beyond the record, have -1 in all four.
 * Per model node m:
 *   hotspot_z2[m]    the smallest z2 over the pairs (u, m): +inf for a node in no pair and for m >= n_nodes
 *   hotspot_node[m]  the lowest u that attains it; -1 without a pair
 *   occupied_fp      bit m % 64 of word m / 64 is set iff some pair (u, m) passes - the format pmx_fingerprint_tanimoto and
 *                    pmx_fingerprint_leaders take
 * Per row:
 *   summary[0]  fit = sum_u node_fit[u]          summary[1]  ideal = sum_u W_u (fit / ideal is 1 with every node on all its hotspots)
 *   summary[2]  best_fit = sum_u node_best[u]    summary[3]  best_ideal = sum_u w of u's best pair
 *               each sum has lane u's value at lane u and 0 for a node without a pair, and is added up by the fixed butterfly of 64 lanes
 *               (at step k = 1, 2, 4, .. 32 lanes i and i ^ k both form v_i + v_(i ^ k))
 *   count       {nodes with a pair, pairs, nodes in place, passing pairs}
 * Outputs, per row:
 *   summary_dev  double [n][4]     count_dev  int32 [n][4]
 *   node_fit_dev, node_best_dev, node_z2_dev  double [n][PMX_MAX_LIGAND_NODES]     node_target_dev  int32 [n][PMX_MAX_LIGAND_NODES]
 *   hotspot_z2_dev  double [n][PMX_MAX_MODEL_NODES]     hotspot_node_dev  int32 [n][PMX_MAX_MODEL_NODES]
 *   occupied_fp_dev  uint64 [n][PMX_FINGERPRINT_WORDS]
 *   status_dev   int32 [n]  PMX_LIGAND_OK; PMX_LIGAND_UNSUPPORTED and PMX_LIGAND_KEY_INVALID as pmx_pose_clash gives them in node mode (an
 *                index outside the library, a record pmx_score reports unsupported; a conformer that is none of the ligand's, a motion value
 *                that is not finite); in key mode also as pmx_align gives them (a level of too many candidates; a match that is no
 *                candidate of its level)
 * A row that is not OK has NaN in summary and in the three per-node doubles, -1 in node_target and hotspot_node, NaN in hotspot_z2, counts
 * of 0 and an empty set. A valid row without pairs has zeros in summary and count. The number is no docking score: it knows no direction,
 * no clash and no atom, and it is not the reference's score.
 * n <= PMX_EXPLAIN_MAX (otherwise PMX_ERR_INVALID); n = 0 succeeds and writes nothing. With n > 0 only key_dev may be NULL. Model and
 * library are on one device, and the pointers are memory of it. Stream-ordered (enqueued, no synchronisation), no allocation, no work
 * buffer, no atomic: the same bits on every run, and for a row wherever it stands in a call. One wavefront per row: a lane per ligand
 * node, the model nodes walked in ascending order by all lanes together, so a lane's sums run in the specified order; the minimum per
 * model node is a cross-lane minimum of (z2, u) under a total order.
 */
int pmx_pose_fit(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES],
                 const double *node_center_dev /* [n_nodes][3] */, const double *node_sigma_dev /* [n_nodes] */,
                 const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint8_t *key_dev /* [n][PMX_MAX_LEVELS] or NULL */,
                 const double *rot_dev /* [n][9] */, const double *trans_dev /* [n][3] */, uint32_t n,
                 double *summary_dev /* [n][4] */, int32_t *count_dev /* [n][4] */,
                 double *node_fit_dev /* [n][64] */, double *node_best_dev /* [n][64] */, double *node_z2_dev /* [n][64] */, int32_t *node_target_dev /* [n][64] */,
                 double *hotspot_z2_dev /* [n][256] */, int32_t *hotspot_node_dev /* [n][256] */,
                 uint64_t *occupied_fp_dev /* [n][PMX_FINGERPRINT_WORDS] */, int32_t *status_dev, void *stream);

/*
 * Shape overlap with a known ligand (pmx_pose_shape.hip): does a posed hit fill the volume a known binder fills? Every other pose call
 * judges a pose against the protein or the model's hotspots; this one judges it against a reference ligand in the pocket's frame: the
 * first-order Gaussian volume overlap of Grant and Pickup (atom-centred Gaussians of amplitude p = 2 sqrt 2), the shape Tanimoto and the
 * two Tversky fractions, nearest-atom distances both ways, and the atom-for-atom RMSD where the two atom lists are one molecule's. The
 * pose is judged where it is: nothing is moved. The reference has no counterpart; the specification is this comment, and
 * tests/shape_ref.py restates it in NumPy.
 *
 * The reference ligand: pmx_shape_ref_create copies 1 <= m <= PMX_MAX_LIGAND_ATOMS atoms - float32 positions xyz[m][3] in the pocket's
 * frame, radii radius[m] - to `device`. Every coordinate must be finite and every radius finite and > 0: anything else is PMX_ERR_INVALID,
 * checked on the host before anything is copied. The handle keeps the atoms widened to float64, each atom's alpha (below) and O_BB, the
 * self-overlap of the reference: the O_AA (below) of the reference's own atoms and radii taken as a point-mode row under the identity
 * motion, computed once at create by the kernel of pmx_pose_shape - the same term order, lane assignment and butterfly as any row, so the
 * two are equal bit for bit. The copy and O_BB are finished when the call returns. pmx_shape_ref_self hands O_BB out;
 * pmx_shape_ref_destroy frees the handle (NULL is allowed).
 *
 * Rows: the two sources of points (node mode, point mode - the three point-mode arguments are what pmx_atoms_gather writes), the posed
 * point p_k = ((R[k][0] x_0 + R[k][1] x_1) + R[k][2] x_2) + t_k and the status rules are exactly pmx_pose_clash's, with two more rules: a
 * row with a point whose radius is not finite or is <= 0 gets PMX_LIGAND_KEY_INVALID (node mode: point_radius; point mode:
 * point_radius_dev[.], or point_radius where that pointer is NULL; a row without points has no such point), and a point-mode row of more
 * than PMX_MAX_LIGAND_ATOMS points gets PMX_LIGAND_UNSUPPORTED (no row of pmx_atoms_gather is one).
 * Arithmetic, float64 with every operation rounded (no fused multiply-add), float32 inputs widened. Constants, as literals:
 * KAPPA = 2.4179879310247046 (pi (3 p / 4 pi)^(2/3)), PI = 3.141592653589793; p^2 is exactly 8.0.
 *   alpha of a radius r   alpha = KAPPA / ((double)r * (double)r)
 *   pair term             a posed point p with alpha_a, an atom (or posed point) at y with alpha_b: e = p - y;
 *                         d2 = (e_0 e_0 + e_1 e_1) + e_2 e_2; s = alpha_a + alpha_b; q = PI / s; k = (alpha_a * alpha_b) / s;
 *                         V = (8.0 * (q * sqrt(q))) * exp(-(k * d2))
 *                         Everything but exp is a correctly rounded operation: a restatement differs from the device through exp alone.
 * Per posed point a of the row:
 *   cross_a    the sum of V over the reference atoms in ascending b
 *   self_a     the sum of V over all points a' of the row in ascending a', a itself included (d2 = 0: the term's prefactor)
 *   near2_a    the smallest d2 to a reference atom; point_ref[a] the lowest b that attains it; point_near[a] = sqrt(near2_a)
 * Per reference atom b < m:
 *   ref_near2_b  the smallest d2 over the row's points, d2 formed from e = p - y exactly as above, so that both sides see the same bits;
 *                ref_point[b] the lowest a that attains it; ref_near[b] = sqrt(ref_near2_b). For a row without points, and for b >= m,
 *                these are +inf and -1.
 * Row sums: each has a lane's points (point % 64) in ascending order, the 64 lanes by the fixed butterfly (at step k = 1, 2, 4, .. 32 lanes
 * i and i ^ k both form v_i + v_(i ^ k)):
 *   O_AB = the sum of cross_a     O_AA = the sum of self_a     S_A = the sum of near2_a     S_B = the sum of ref_near2_b (lane b % 64)
 *   S_O  = when the row has exactly m points, the sum of |p_a - y_a|^2, point a against reference atom a
 * Outputs, per row:
 *   summary_dev  double [n][10]  [0] O_AB  [1] O_AA  [2] O_BB
 *                                [3] O_AB / ((O_AA + O_BB) - O_AB), the shape Tanimoto
 *                                [4] O_AB / O_BB: how much of the known ligand the row fills
 *                                [5] O_AB / O_AA: how much of the row lies inside it; 0 where O_AA is 0
 *                                [6] sqrt(S_A / points), NaN without a point   [7] sqrt(S_B / m), +inf without a point
 *                                [8] sqrt(S_O / m) when points == m, otherwise NaN   [9] 0
 *   count_dev    int32 [n][4]    [0] points; [1] points with near2_a < c2; [2] reference atoms with ref_near2_b < c2; [3] m;
 *                                c2 = (double)cover * (double)cover
 *   point_near_dev, point_ref_dev  double / int32 in the layout of pmx_pose_clash's point_pen_dev / point_atom_dev: node mode
 *                                [n][PMX_MAX_LIGAND_NODES] with NaN / -1 beyond the record's nodes; point mode the layout of the points
 *   ref_near_dev  double [n][PMX_MAX_LIGAND_ATOMS]     ref_point_dev  int32 [n][PMX_MAX_LIGAND_ATOMS]
 *   status_dev   int32 [n]
 * A row that is not OK has NaN in all of summary, counts of 0 (all four), NaN / -1 for every point it has room for and NaN / -1 in all of
 * its ref_near / ref_point.
 * Three consequences are exact. (i) A row whose points are the reference's own atoms, in order, with the same radii, under the identity
 * motion (where the posed point equals the input exactly) has O_AB == O_AA == O_BB bit for bit and therefore Tanimoto exactly 1.0, every
 * near 0 and summary[8] == 0. (ii) One point on one reference atom gives exactly 8.0 * (q * sqrt(q)). (iii) A row far from the reference
 * has O_AB == 0 through underflow, and Tanimoto exactly 0.
 * The first-order overlap counts every pair once and subtracts nothing for triples, so O_AA over-counts a molecule's volume; the excess
 * largely cancels in the three ratios and not in the absolute volumes.
 * n <= PMX_EXPLAIN_MAX (otherwise PMX_ERR_INVALID); n = 0 succeeds and writes nothing. With n > 0 no output may be NULL. point_radius
 * and cover must be finite, cover >= 0. In node mode the library is on the reference's device; the pointers are memory of that device.
 * Stream-ordered (enqueued, no synchronisation), no allocation, no work buffer, no atomic: the same bits on every run, and for a row
 * wherever it stands in a call. One wavefront per row, every pair evaluated (no cut-off by distance): points * (m + points) exp a row.
 */
typedef struct pmx_shape_ref pmx_shape_ref;
int pmx_shape_ref_create(const float *xyz /* [m][3] */, const float *radius /* [m] */, uint32_t m, int device, pmx_shape_ref **out);
int pmx_shape_ref_self(const pmx_shape_ref *ref, double *self_out);
int pmx_shape_ref_destroy(pmx_shape_ref *ref);
int pmx_pose_shape(const pmx_shape_ref *ref, const pmx_library *lib /* NULL in point mode */, const uint64_t *ligands_dev, const int32_t *conformer_dev /* node mode: [n] each */,
                   const uint64_t *point_off_dev /* [n + 1] */, const float *points_dev /* [.][3] */, const float *point_radius_dev /* [.] or NULL */,
                   const double *rot_dev /* [n][9] */, const double *trans_dev /* [n][3] */, uint32_t n, float point_radius, float cover,
                   double *summary_dev /* [n][10] */, int32_t *count_dev /* [n][4] */, double *point_near_dev, int32_t *point_ref_dev,
                   double *ref_near_dev /* [n][PMX_MAX_LIGAND_ATOMS] */, int32_t *ref_point_dev /* [n][PMX_MAX_LIGAND_ATOMS] */, int32_t *status_dev, void *stream);

/*
 * Shape overlay (pmx_shape_overlay.hip): pmx_pose_shape judges a pose where it stands; these two calls move it. pmx_shape_overlay maximises
 * a row's O_AB over its rigid motion from the motion it is given - a rigid motion changes neither O_AA nor O_BB, so that also maximises the
 * shape Tanimoto - and pmx_shape_starts gives a row the four motions that lay its inertial frame on the reference's, so that an overlay
 * need not start from a pose at all. Rigid only, shape only (no atom types, no hydrogens), unweighted frames, and a local maximum: the one
 * the start leads to. The reference has no counterpart; the specification is this comment, and tests/overlay_ref.py restates it in NumPy.
 *
 * Rows: the sources of points (node mode, point mode, what pmx_atoms_gather writes), the pmx_shape_ref handle, the radius rules and the
 * status rules are exactly pmx_pose_shape's. Arithmetic is float64 with every operation rounded, float32 inputs widened.
 *
 * pmx_shape_overlay. Evaluation at a motion (R, t): the posed points by pmx_pose_clash's formula from the stored (R, t); c = their sum (a
 * lane's points, point % 64, ascending; the fixed butterfly; each coordinate) / the number of points, as pmx_pose_refine's. For a posed
 * point a and a reference atom b, e, d2, k and V are exactly the pair term of the pmx_pose_shape comment, and kappa = (2.0 * k) * V. Per
 * point, each a running sum in ascending b:
 *   cross_a = the sum of V     f_a = the sum of kappa * e (each component)     w_a = the sum of kappa
 * O_AB = the sum of cross_a as pmx_pose_shape sums it (a lane's points ascending, the butterfly); E = -O_AB. f_a is the exact gradient of E
 * in p_a. With r = p_a - c and a small motion delta p = omega x r + tau, the exact gradient is g = the sum over a of [r x f_a, f_a] and the
 * surrogate Hessian H = the sum over a of the closed-form anchor blocks of pmx_pose_refine with k = w_a: w_a (|r|^2 I - r r^T), w_a [r]_x,
 * w_a I, formed once per point, operation for operation as there (rr = (r_0 r_0 + r_1 r_1) + r_2 r_2; w (rr - r_0 r_0); w * -(r_0 r_1);
 * w * -r_2; .. ; g_0 = r_1 f_2 - r_2 f_1, ..), a lane's points ascending, the butterfly per value. H is positive semidefinite: it is the
 * curvature of the quadratic that bounds -V from above at the current d2 (-exp(-k d2) is concave in d2).
 * Iteration: pmx_pose_refine's with the same constants, on E = -O_AB:
 *   1. evaluate at the start motion; O_AA once, from the points posed there, in pmx_pose_shape's order
 *   2. the row has no point, or O_AB is not > 0 (a row far away: every term underflows): stop, reason 0 - the outputs are the input motion
 *      bit for bit
 *   3. otherwise lambda = 1e-3, and while iterations < max_iter:
 *        solve (H + lambda diag(H_ii + 1e-9)) delta = -g by Cholesky; omega = delta[0 .. 3), tau = delta[3 .. 6)
 *        Rd = Rodrigues of omega as in pmx_pose_refine; trial: R' = Rd R, t' = Rd (t - c) + c + tau; evaluate there; ++iterations
 *        O_AB' > O_AB: accept, lambda = max(lambda / 4, 1e-9); if O_AB' - O_AB <= ftol * O_AB (the value before the step): stop, reason 1
 *        otherwise: lambda *= 8; if lambda > 1e8: stop, reason 3
 *      (a pivot that is not positive, or a delta that is not finite, is a rejected trial: an iteration without an evaluation)
 *   4. running out of max_iter: reason 2. 0 <= max_iter <= PMX_REFINE_MAX_ITER; max_iter = 0 evaluates once and returns the start.
 * A row that starts exactly at a maximum has g = 0 up to rounding, no trial raises O_AB, and it ends with reason 3 after about 13 rejected
 * trials (1e-3 * 8^13 > 1e8), not with reason 1. No loop depends on convergence.
 * Outputs, per row:
 *   rot_out_dev, trans_out_dev   double [n][9], [n][3]: the last accepted motion
 *   energy_dev   double [n][8]   O_AB at the start, O_AB final, O_AA, O_BB (the handle's), the Tanimoto O_AB / ((O_AA + O_BB) - O_AB) at
 *                                the start and final, the net rotation angle from the start in rad (0 when no step was accepted),
 *                                |c_final - c_start|
 *   count_dev    int32 [n][4]    iterations, accepted steps, stop reason, points
 *   status_dev   int32 [n]       PMX_LIGAND_*
 * A row that is not OK has NaN motions and energies, counts of 0 and a stop reason of -1.
 * Cross-checks, bit for bit: energy[0] and energy[2] are pmx_pose_shape's summary[0] and summary[1] at the input motion; energy[1] is its
 * summary[0] at rot_out / trans_out; O_AB final is never below O_AB at the start.
 * n <= PMX_EXPLAIN_MAX (otherwise PMX_ERR_INVALID); n = 0 succeeds and writes nothing. ftol >= 0 and finite, point_radius finite; one
 * source of points per call; no output may be NULL. Stream-ordered (enqueued, no synchronisation), no allocation, no work buffer, no
 * atomic: the same bits on every run, and for a row wherever it stands in a call. One wavefront per row; an evaluation is points * m exp.
 *
 * pmx_shape_starts. The frame of a point set - the row's unposed points, or the reference's atoms; unweighted:
 *   centre   the sum of the points (a lane's points, index % 64, ascending; the butterfly; each coordinate) / their number
 *   S        the six sums xx, xy, xz, yy, yz, zz of d_i d_j, d = x - centre, summed the same way
 *   Jacobi   A = the symmetric 3 x 3 of S, V = I; PMX_SHAPE_JACOBI_SWEEPS sweeps over the pairs (p, q) = (0,1), (0,2), (1,2), r the third
 *            index; a pair whose A_pq is exactly 0 is skipped; otherwise theta = (A_qq - A_pp) / (2.0 * A_pq);
 *            at = |theta| + sqrt(theta * theta + 1.0); tn = 1.0 / at for theta >= 0, otherwise -1.0 / at; cc = 1.0 / sqrt(tn * tn + 1.0);
 *            ss = tn * cc; A_pp -= tn * A_pq; A_qq += tn * A_pq (the old A_pq in both); A_pq = 0;
 *            (A_rp, A_rq) = (cc * A_rp - ss * A_rq, ss * A_rp + cc * A_rq); every row k of V: (V_kp, V_kq) = (cc * V_kp - ss * V_kq,
 *            ss * V_kp + cc * V_kq). Only + - * / and sqrt: a restatement has the same bits.
 *   axes     the columns of V by descending A_ii, equal values keeping the lower index; the third axis is replaced by the cross product
 *            of the first two, so the frame is right-handed. A set of no points has the identity frame at the origin.
 * Start s = start_dev[i] of row i, with a_k the row's axes and centre c_A, b_k and c_B the reference's: D_0 = I, D_s the half turn about
 * axis s - 1 (signs d = (1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1));
 *   R_ij = (d_0 (b_0i a_0j) + d_1 (b_1i a_1j)) + d_2 (b_2i a_2j)      t_i = c_Bi - ((R_i0 c_A0 + R_i1 c_A1) + R_i2 c_A2)
 * frame_dev double [n][16]: the row's centre [0..3), axis k at [3 + 3 k ..), the three sorted A_ii (sums, not divided by the number) at
 * [12..15), [15] 0. A start outside 0 .. 3 gives the row PMX_LIGAND_KEY_INVALID; a point-mode row of more than PMX_MAX_LIGAND_ATOMS points
 * PMX_LIGAND_UNSUPPORTED; a row that is not OK has NaN in rot_out, trans_out and frame. The same limits and ordering rules as above.
 */
#define PMX_SHAPE_JACOBI_SWEEPS 8
int pmx_shape_overlay(const pmx_shape_ref *ref, const pmx_library *lib /* NULL in point mode */, const uint64_t *ligands_dev, const int32_t *conformer_dev,
                      const uint64_t *point_off_dev, const float *points_dev, const float *point_radius_dev, const double *rot_dev, const double *trans_dev,
                      uint32_t n, float point_radius, double ftol, int max_iter, double *rot_out_dev /* [n][9] */, double *trans_out_dev /* [n][3] */,
                      double *energy_dev /* [n][8] */, int32_t *count_dev /* [n][4] */, int32_t *status_dev, void *stream);
int pmx_shape_starts(const pmx_shape_ref *ref, const pmx_library *lib /* NULL in point mode */, const uint64_t *ligands_dev, const int32_t *conformer_dev,
                     const uint64_t *point_off_dev, const float *points_dev, const int32_t *start_dev /* [n] */, uint32_t n, double *rot_out_dev /* [n][9] */,
                     double *trans_out_dev /* [n][3] */, double *frame_dev /* [n][16] */, int32_t *status_dev, void *stream);

/*
 * Colour overlap (pmx_colour.hip): the two shape calls above compare untyped spheres - "shape only". These calls add the typed term, the
 * "colour" of ligand-based screening: does a posed hit put its pharmacophore features - the typed nodes every library record carries - where
 * a known binder has features of the same type? pmx_pose_colour judges a pose where it stands, pmx_combo_overlay moves a row by shape and
 * colour together. No direction is compared - no donor / acceptor vector, no ring normal - and no hydrogens: a feature is a point with a
 * set of types. The overlaps are first-order as the shape term's. The reference has no counterpart; the specification is this comment,
 * and tests/colour_ref.py and tests/combo_ref.py restate it in NumPy.
 *
 * The colour reference: pmx_colour_ref_create copies 1 <= f <= PMX_MAX_LIGAND_NODES features of the known ligand - float32 positions
 * xyz[f][3] in the pocket's frame, type masks typemask[f] (bit t is type t; every mask < 128; a mask of 0 is allowed: such a feature pairs
 * with nothing) - with the type weights weights[PMX_NUM_TYPES] (finite, >= 0) and one radius (finite, > 0) to `device`. Anything else is
 * PMX_ERR_INVALID, checked on the host before anything is copied. The handle keeps the features widened to float64, the weights as doubles,
 * alpha_c = KAPPA / ((double)radius * (double)radius) and C_BB, the self-overlap of the reference: the C_AA (below) of the reference's own
 * features and masks taken as a feature-mode row under the identity motion, computed once at create by the kernel of pmx_pose_colour, so the
 * two are equal bit for bit. The copy and C_BB are finished when the call returns. pmx_colour_ref_self hands C_BB out;
 * pmx_colour_ref_destroy frees the handle (NULL is allowed).
 *
 * The pair term. A posed typed point a with mask ma and a feature (or posed typed point) b with mask mb:
 *   w = the sum, in ascending type t, of (double)weights[t] over the bits set in ma & mb, from 0.0
 *   a pair with w == 0 is left out (of every sum, and of every nearest-partner search: such a pair shares no weighted type)
 *   otherwise V = the pair term of the pmx_pose_shape comment with alpha_a = alpha_b = alpha_c (e = p - y, d2, s, q, k, V in its order),
 *   and the pair's term is w * V
 * Arithmetic is float64 with every operation rounded (no fused multiply-add), float32 inputs widened; the posed point is pmx_pose_clash's.
 * All terms are >= 0 because the weights are: a restatement differs from the device through exp alone.
 *
 * pmx_pose_colour. Rows come from one of two sources, never both: node mode (lib, ligands_dev, conformer_dev: the record's nodes at
 * that conformer with the record's type masks) or feature mode (lib NULL; feat_off_dev [n + 1], feat_xyz_dev [.][3], feat_mask_dev [.]:
 * typed points of the caller's, row i holding points feat_off[i] .. feat_off[i + 1]). The status rules are pmx_pose_clash's, with two more:
 * a row of more than PMX_MAX_LIGAND_NODES typed points gets PMX_LIGAND_UNSUPPORTED, a row with a mask >= 128 PMX_LIGAND_KEY_INVALID (a
 * record of an uploaded library has no such mask: pmx_library_upload neutralises a record that has one, and its rows are
 * PMX_LIGAND_UNSUPPORTED).
 * Per typed point a of the row (lane a):
 *   cross_a    the sum of w * V over the features in ascending b
 *   cross_a^t  for each type t, the sum of weights[t] * V over the features in ascending b whose pair with a shares t (and has w != 0)
 *   self_a     the sum of w * V over all points a' of the row in ascending a', a itself included
 *   near2_a    the smallest d2 to a feature whose pair with a has w != 0; node_feature[a] the lowest b that attains it, -1 if there is none
 * Per feature b < f (lane b): feat_near2_b, the smallest d2 (from e = p - y, as above) over the row's points whose pair with b has
 * w != 0; feat_node[b] the lowest a that attains it, -1 if there is none.
 * Row sums: lane a holds point a (a row has at most 64), the 64 lanes are summed by the fixed butterfly of pmx_pose_shape:
 *   C_AB = the sum of cross_a     C_AA = the sum of self_a     C_AB^t = the sum of cross_a^t     S = the sum of near2_a over the matched
 *   points, those with node_feature[a] >= 0
 * The C_AB^t add up to C_AB only up to rounding: a pair's w is rounded once as a sum of weights, its parts are rounded one by one.
 * Outputs, per row:
 *   summary_dev       double [n][8]   [0] C_AB  [1] C_AA  [2] C_BB (the handle's)
 *                                     [3] the colour Tanimoto C_AB / ((C_AA + C_BB) - C_AB), and 0 where C_AB == 0
 *                                     [4] C_AB / C_BB, 0 where C_BB is 0     [5] C_AB / C_AA, 0 where C_AA is 0
 *                                     [6] sqrt(S / matched points), NaN where none is matched     [7] 0
 *   type_overlap_dev  double [n][PMX_NUM_TYPES]   C_AB^t
 *   count_dev         int32 [n][4]    [0] points; [1] points with node_feature[a] >= 0 and near2_a < c2; [2] features with feat_node[b] >= 0
 *                                     and feat_near2_b < c2; [3] f;   c2 = (double)cover * (double)cover
 *   node_colour_dev, node_near_dev  double [n][64]: cross_a and sqrt(near2_a) - NaN for a point without a partner, and beyond the row's points
 *   node_feature_dev  int32 [n][64]   (-1 beyond the row's points)
 *   feat_near_dev, feat_node_dev    double / int32 [n][64]: sqrt(feat_near2_b) and feat_node[b]; NaN / -1 without a partner and for b >= f
 *   matched_fp_dev    uint64 [n][PMX_FINGERPRINT_WORDS]: bit b of word 0 is set where feature b is counted in count[2]; the other words are 0.
 *                     The format pmx_fingerprint_tanimoto and pmx_fingerprint_leaders take: hits can be clustered by which of the
 *                     binder's interactions they reproduce
 *   status_dev        int32 [n]
 * A row that is not OK has NaN in all of summary, type_overlap, node_colour, node_near and feat_near, -1 in node_feature and feat_node,
 * counts of 0 (all four) and an empty matched_fp.
 * Exact consequences. (i) The reference's own features, in order, under the identity motion give C_AB == C_AA == C_BB bit for bit and a
 * Tanimoto of exactly 1.0 (where C_BB > 0). (ii) One point on one feature of a shared weighted type gives exactly w * (8.0 * (q * sqrt(q))),
 * q = PI / (alpha_c + alpha_c). (iii) A row far from the reference has C_AB == 0 through underflow and Tanimoto exactly 0. (iv) A row
 * whose types are all zero-weighted, or shared with no feature, has C_AB == 0 and Tanimoto 0.
 *
 * pmx_combo_overlay maximises F = O_AB + colour_weight * C_AB over the rigid motion of a row. It takes a pmx_shape_ref and a
 * pmx_colour_ref on one device and a library on that device, which is always required: the colour points are the record's nodes (ligand
 * ligands_dev[i], conformer conformer_dev[i]) with the record's masks. The shape points are those same nodes with point_radius (the point
 * triple NULL) or the point triple - what pmx_atoms_gather writes for the same (ligand, conformer) rows. Both point sets move under the
 * one motion. The status rules are pmx_shape_overlay's for the shape points and pmx_pose_colour's for the nodes; the nodes' status comes
 * first.
 * Evaluation at (R, t): O_AB, c (the centroid of the posed shape points; 0 where there is none), H_shape and g_shape are exactly
 * pmx_shape_overlay's. For the node a of lane a and a feature b with w != 0: e, d2, k and V are the pair term above, Vw = w * V,
 * kappa = (2.0 * k) * Vw; in ascending b, cross_a = the sum of Vw, f_a = the sum of kappa * e, w_a = the sum of kappa. C_AB = the butterfly
 * of the cross_a: pmx_pose_colour's bits. With r = p_a - c the node's block of H_colour and g_colour is the closed form of the shape term,
 * operation for operation (w_a (rr - r_0 r_0); w_a * -(r_0 r_1); ..; g_0 = r_1 f_2 - r_2 f_1; ..), each value 0.0 + the block's (a lane
 * has one node), then the butterfly per value. After the butterflies H = H_shape + colour_weight * H_colour and g = g_shape +
 * colour_weight * g_colour, value by value (the six values of H that are 0 by structure stay 0); F = O_AB + colour_weight * C_AB.
 * Iteration: pmx_shape_overlay's, on F: follow only when F > 0 at the start (otherwise reason 0, the input's bits); accept when F' > F;
 * stop with reason 1 when F' - F <= ftol * F. With colour_weight = 0 every decision and every bit of the motion is pmx_shape_overlay's.
 * colour_weight is finite and >= 0; it is uncalibrated - the Python layer's default only balances the two self-overlaps.
 * Outputs, per row:
 *   rot_out_dev, trans_out_dev   double [n][9], [n][3]: the last accepted motion
 *   energy_dev   double [n][16]  O_AB at the start, O_AB final, O_AA, O_BB, the shape Tanimoto at the start and final; C_AB at the start, C_AB
 *                                final, C_AA (pmx_pose_colour's, of the nodes posed at the input motion), C_BB, the colour Tanimoto at the
 *                                start and final (0 where C_AB == 0); combo at the start and final, the sum of the two Tanimotos, between
 *                                0 and 2; the net rotation angle from the start in rad; |c_final - c_start|
 *   count_dev    int32 [n][6]    iterations, accepted steps, stop reason, shape points, nodes, f
 *   status_dev   int32 [n]
 * A row that is not OK has NaN motions and energies, counts of 0 and a stop reason of -1.
 * Cross-checks, bit for bit: energy[6] and energy[8] are pmx_pose_colour's summary[0] and summary[1] at the input motion, energy[7] its
 * summary[0] at rot_out / trans_out; energy[0], [1] and [2] are pmx_pose_shape's as for pmx_shape_overlay; F final is never below F at
 * the start.
 * Both calls: n <= PMX_EXPLAIN_MAX (otherwise PMX_ERR_INVALID); n = 0 succeeds and writes nothing; with n > 0 no output may be NULL. cover is
 * finite and >= 0; ftol and max_iter as pmx_shape_overlay's. Stream-ordered (enqueued, no synchronisation), no allocation, no work buffer,
 * no atomic: the same bits on every run, and for a row wherever it stands in a call. One wavefront per row.
 */
typedef struct pmx_colour_ref pmx_colour_ref;
int pmx_colour_ref_create(const float *xyz /* [f][3] */, const uint8_t *typemask /* [f] */, uint32_t f, const float weights[PMX_NUM_TYPES], float radius, int device,
                          pmx_colour_ref **out);
int pmx_colour_ref_self(const pmx_colour_ref *ref, double *self_out);
int pmx_colour_ref_destroy(pmx_colour_ref *ref);
int pmx_pose_colour(const pmx_colour_ref *ref, const pmx_library *lib /* NULL in feature mode */, const uint64_t *ligands_dev, const int32_t *conformer_dev /* node mode: [n] each */,
                    const uint64_t *feat_off_dev /* [n + 1] */, const float *feat_xyz_dev /* [.][3] */, const uint8_t *feat_mask_dev /* [.] */,
                    const double *rot_dev /* [n][9] */, const double *trans_dev /* [n][3] */, uint32_t n, float cover, double *summary_dev /* [n][8] */,
                    double *type_overlap_dev /* [n][PMX_NUM_TYPES] */, int32_t *count_dev /* [n][4] */, double *node_colour_dev /* [n][64] */, double *node_near_dev /* [n][64] */,
                    int32_t *node_feature_dev /* [n][64] */, double *feat_near_dev /* [n][64] */, int32_t *feat_node_dev /* [n][64] */,
                    uint64_t *matched_fp_dev /* [n][PMX_FINGERPRINT_WORDS] */, int32_t *status_dev, void *stream);
int pmx_combo_overlay(const pmx_shape_ref *shape, const pmx_colour_ref *colour, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev,
                      const uint64_t *point_off_dev /* NULL: the nodes are the shape points */, const float *points_dev, const float *point_radius_dev, const double *rot_dev,
                      const double *trans_dev, uint32_t n, float point_radius, double colour_weight, double ftol, int max_iter, double *rot_out_dev /* [n][9] */,
                      double *trans_out_dev /* [n][3] */, double *energy_dev /* [n][16] */, int32_t *count_dev /* [n][6] */, int32_t *status_dev, void *stream);

/*
 * Retrospective validation (pmx_enrich.hip): does a model, under given type weights, rank known binders above decoys? Per column of scores
 * over one labelled list, and per bootstrap resample of the list, the integers and sums from which the host derives AUROC, enrichment
 * factors and BEDROC. The specification is this comment (the reference has no counterpart); tests/enrichment_ref.py restates it in NumPy.
 *
 *   scores_dev   float32 [n_cols][col_stride], the first n of each row are used; 1 <= n < 2^31, 1 <= n_cols <= PMX_ENRICH_MAX_COLUMNS
 *   status_dev   int32 [n] or NULL: PMX_LIGAND_*
 *   labels_dev   uint8 [n]: 0 decoy, 1 active, 2 not counted. Any other value refuses the call - which is stream-ordered and reads nothing
 *                back, so the refusal is written where the caller will read: every entry of totals is UINT64_MAX and the other outputs are
 *                undefined
 *   cut_ppm      uint32 [n_cut] in host memory (read before the call returns): cutoffs in parts per million of the list, each 1 .. 10^6;
 *                n_cut <= PMX_ENRICH_MAX_CUTOFFS
 *   alpha > 0    BEDROC's alpha;   n_boot <= PMX_ENRICH_MAX_BOOTSTRAP resamples;   seed of the bootstrap
 *
 * The ranked list of a column. Counted are the ligands labelled 0 or 1, N' of them. They are ranked by descending score, equal scores in
 * ascending ligand index. A NaN score or a non-zero status counts as -inf (ranked last, tied with each other and with a score of -inf);
 * -0.0 and +0.0 are one value. A tie group is a maximal run of equal scores. Every output but `order` is the expectation under random
 * tie-breaking, so the order inside a group has no effect on it.
 *
 * Weights. Row 0 of every output is the sample: c_i = 1. Row b = 1 .. n_boot is a Poisson bootstrap resample: c_i = Poisson(1) from a
 * counter-based hash of (seed, b, i), the same in every column (differences between columns are paired). Arithmetic mod 2^64:
 *   mix(x):  x ^= x >> 30;  x *= 0xBF58476D1CE4E5B9;  x ^= x >> 27;  x *= 0x94D049BB133111EB;  x ^= x >> 31
 *   h = mix(mix(seed + 0x9E3779B97F4A7C15 * b) + i)
 *   c_i = the number of entries of T[m] = floor(2^64 * P(Poisson(1) <= m)), m = 0 .. 20, that are <= h  (T[20] = 2^64 - 1: 21 entries)
 * Per group g: a_g, d_g the weighted actives and decoys, c_g = a_g + d_g; A_before, C_before the sums of a_g, c_g over the groups ranked
 * before it. A group with c_g = 0 contributes nothing. N*, n_a*, n_d*: the weighted totals of a row.
 *
 *   totals_dev   uint64 [1 + n_boot][3]            (N*, n_a*, n_d*)
 *   u2_dev       uint64 [n_cols][1 + n_boot]       sum over g of d_g * (2 * A_before + a_g): twice the Mann-Whitney U with ties at one half.
 *                                                  AUROC = u2 / (2 n_a* n_d*)
 *   hits_dev     double [n_cols][1 + n_boot][n_cut]  k = (ppm * N* + 999999) / 1000000 in uint64 (the ceiling). For the group with
 *                                                  C_before < k <= C_before + c_g:  (double)(A_before + a_g) when k = C_before + c_g, else
 *                                                  (double)A_before + (double)a_g * (double)(k - C_before) / (double)c_g, evaluated left to
 *                                                  right, each operation rounded to double (no fused multiply-add). 0 when N* = 0.
 *   expsum_dev   double [n_cols][1 + n_boot]       sum over the groups with a_g > 0 of a_g * E_g, E_g the mean of exp(-alpha r / N*) over the
 *                                                  group's ranks r = C_before + 1 .. C_before + c_g, formed as, with s = -alpha / (double)N*,
 *                                                  (double)a_g * (exp(s * (C_before + 1)) * expm1(s * c_g) * (1 / expm1(s)) / c_g).
 *                                                  Summed in a fixed order without floating-point atomics: a call gives the same bits
 *                                                  every time; against another order of summation it agrees to rounding.
 *   order_dev    int64 [n_cols][order_stride] or NULL: the ranked ligand indices of each column, the first min(N', order_stride) of a row
 *
 * The host derives EF = (hits / k) / (n_a* / N*), BEDROC (Truchon & Bayly 2007, from expsum, n_a*, N*, alpha) and percentile intervals over
 * the rows; a row with no active, no decoy or N* = 0 is NaN there, not an error here. One stable radix sort per column (hipcub), one pass
 * that leaves a byte per ranked position, and one work-group per (column, row) that walks the ranked list in tiles of PMX_ENRICH_TILE
 * positions with a carry from tile to tile. Stream-ordered like pmx_score: enqueued, no synchronisation. The work buffers are kept per device
 * (a call on another stream starts behind the call before it) and freed by pmx_release_workspaces.
 */
#define PMX_ENRICH_MAX_COLUMNS 64
#define PMX_ENRICH_MAX_CUTOFFS 64
#define PMX_ENRICH_MAX_BOOTSTRAP 4096
#define PMX_ENRICH_TILE 2048
int pmx_enrichment(const float *scores_dev, uint64_t col_stride, int n_cols, uint64_t n, const int32_t *status_dev, const uint8_t *labels_dev,
                   const uint32_t *cut_ppm, int n_cut, double alpha, int n_boot, uint64_t seed, uint64_t *totals_dev, uint64_t *u2_dev, double *hits_dev,
                   double *expsum_dev, int64_t *order_dev, uint64_t order_stride, int device, void *stream);
/* HIP-event times of the last pmx_enrichment on `device` that was made with profiling on (pmx_set_profiling(1): events around the phases,
 * nothing else changes): ms_out = {totals, keys + sort (all columns), ranked-byte pass (all columns), walk}. Waits for that call. */
int pmx_enrichment_times(int device, double ms_out[4]);

/* Frees the scoring workspaces libpmx keeps between calls on `device` (synchronises the device first). */
int pmx_release_workspaces(int device);

/* Diagnostics of the last pmx_score / pmx_score_multi on this thread. pmx_score_stats_get synchronises the stream the
 * call ran on (the counters live on the device); the times are HIP-event times and are filled when profiling was on
 * (pmx_set_profiling(1): three event records per super-chunk, nothing else changes). */
typedef struct {
    double ms_total;            /* the call's kernels, first to last */
    double ms_ligand, ms_tasks; /* of the last super-chunk: ligand kernels (tables + tree search within budget) | task rounds + finalize */
    uint64_t ligands_last;      /* ligands in that super-chunk */
    uint64_t n_frames;          /* tree nodes entered (tree.py:15-53); walkers of a split ligand share maxima while they run, so this
                                   count (not the scores) varies a little from run to run */
    uint64_t n_passes;          /* walker passes: evaluations of a frame's candidates (probes included) */
    uint64_t n_items;           /* table phase: (table entry, ligand node pair) evaluations per wavefront, i.e. / (64 / G) slots */
    uint64_t n_exact_cells;     /* items whose 2-sigma majority test was counted term by term (pass set not an interval), per lane */
    uint64_t n_heavy;           /* walks that ran over their budget (ligands and queued subtrees) */
    uint64_t n_tasks;           /* subtrees taken from the task queue (the empty records that pad a shard's end included) */
    uint64_t n_exported;        /* subtree records written to the task queue */
    uint64_t n_slice_overflow;  /* ligands whose tables did not fit a per-wavefront slice */
    uint64_t n_probes, n_probe_passes; /* reachability searches: subtrees below 5 matches that are handed over, or dropped by the bound test */
    uint64_t max_passes;        /* longest single walk */
    uint64_t queue_overflow;    /* 1 if a task queue shard filled up (results stay exact; raise PMX_TASKQ_MB) */
    uint64_t arena_bytes;       /* table arena in use at the end of the last super-chunk */
    uint64_t ticks_scan, ticks_tables, ticks_bounds, ticks_walk, ticks_alive; /* s_memtime ticks summed over wavefronts, by phase */
    uint64_t n_exact_values;    /* self-table items evaluated term by term because their cell of the tabulated function is not accurate relative
                                   to the function's own (tail) value there, per lane */
    uint64_t dbg[8];            /* walker counters of instrumented builds (-DPMX_COUNTERS, _TABLE_TICKS, _WALK_TICKS, _TABLE_FILL: see the list in csrc/pmx_screen_tables.h); 0 otherwise */
    uint64_t n_path_bounds, n_path_drops; /* children tested against the bound their actual path gives (path_bound()), and dropped by it */
    uint64_t n_dead_entries;    /* pair-table entries settled as -1 without computing their items: more than half of their node pairs lie
                                   outside every 2-sigma window of the two model clusters, for every conformer */
    uint64_t arena_capacity;    /* bytes of the table arena this workspace obtained (PMX_ARENA_MB, or a third of the free device memory at its first
                                   allocation, halved until it fit): which ligands can get PMX_LIGAND_TOO_LARGE depends on it */
} pmx_score_stats;
int pmx_score_stats_get(pmx_score_stats *out);
int pmx_set_profiling(int enabled); /* when enabled pmx_score records HIP events around its phases (no synchronisation) */

#ifdef __cplusplus
}
#endif
#endif /* PMX_H */
