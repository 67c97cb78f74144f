/*
 * cda.h — C ABI of the MI355X data-availability engine (libcda.so).
 *
 * Drop-in boundary for celestia-app's DA hot path.  Every entry
 * point takes plain pointers and sizes, returns 0 on success or a negative
 * CDA_E_* code, never aborts, and never retains a caller pointer after it
 * returns (cgo rule).  Each function cites the reference interface it replaces
 * (paths relative to the celestia-app reference tree).
 *
 * Threading: a cda_ctx serialises its own calls with an internal mutex, so the
 * entry points are re-entrant from concurrent goroutines (rsmt2d calls
 * Codec.Encode / Decode / NewTree concurrently per axis); use one ctx per OS
 * thread for parallel submission.  The device-resident entry points (..._device)
 * enqueue on the caller's stream but share the ctx's workspace: the ctx orders
 * them after its earlier work and every later call after them (events), so
 * mixing them with the synchronous calls is safe.
 */
#ifndef CDA_H
#define CDA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CDA_SHARE_SIZE 512    /* appconsts.ShareSize, pkg/appconsts/global_consts.go:29 */
#define CDA_NAMESPACE_SIZE 29 /* appconsts.NamespaceSize, global_consts.go:26 */
#define CDA_NODE_SIZE 90      /* NMT node = min ns ‖ max ns ‖ sha256 (test/util/malicious/app_test.go:58) */
#define CDA_HASH_SIZE 32

enum {
  CDA_OK = 0,
  CDA_E_NOT_POW2 = -1,     /* da.ExtendShares "number of shares is not a power of 2" (data_availability_header.go:67-69) */
  CDA_E_NOT_SQUARE = -2,   /* rsmt2d newDataSquare "number of chunks must be a square number" */
  CDA_E_SHARD_SIZE = -3,   /* LeoRSCodec.ValidateChunkSize: chunk size % 64 != 0 / uneven chunks */
  CDA_E_NS_SHORT = -4,     /* wrapper Push "data is too short to contain namespace ID" (nmt_wrapper.go:97-99) */
  CDA_E_NS_ORDER = -5,     /* nmt ErrInvalidPushOrder (leaf namespaces must be non-decreasing) */
  CDA_E_TOO_FEW = -6,      /* reedsolomon ErrTooFewShards (Decode with < k shards) */
  CDA_E_UNREPAIRABLE = -7, /* rsmt2d ErrUnrepairableDataSquare */
  CDA_E_BYZANTINE = -8,    /* rsmt2d ErrByzantineData{Axis, Index} */
  CDA_E_ARG = -9,          /* invalid argument (null pointer, k out of range, ...) */
  CDA_E_DEVICE = -10,      /* HIP runtime / device failure */
  CDA_E_PUSH_PAST = -11,   /* wrapper Push "pushed past predetermined square size" (nmt_wrapper.go:94-96) */
  CDA_E_UNSUPPORTED = -12, /* configuration not implemented on the device path */
  CDA_E_SHARE_VERSION = -13, /* x/blob ErrUnsupportedShareVersion (appconsts.SupportedShareVersions = {0}) */
  CDA_E_BLOB_SIZE = -14,     /* x/blob ErrZeroBlobSize: empty blob data (x/blob/types/payforblob.go:230-232) */
  CDA_E_NOMEM = -15,         /* host allocation failed inside the library (std::bad_alloc caught at the C ABI) */
  CDA_E_INTERNAL = -16,      /* any other C++ exception caught at the C ABI (e.g. a helper thread failed to start);
                                no exception ever crosses an entry point (app/process_proposal.go:28-34 recovers
                                Go panics only) */
};

enum { CDA_AXIS_ROW = 0, CDA_AXIS_COL = 1 }; /* rsmt2d.Row / rsmt2d.Col */

typedef struct cda_ctx cda_ctx;

/* Detail for NS_ORDER / BYZANTINE / NS_SHORT errors (mirrors rsmt2d.ErrByzantineData
 * and nmt's push-order error: which axis/index and which leaf). */
typedef struct {
  int32_t code;
  int32_t axis;  /* CDA_AXIS_ROW / CDA_AXIS_COL, or -1 */
  int32_t index; /* axis index, or -1 */
  int32_t leaf;  /* leaf (share) index within the axis, or -1 */
  int32_t block; /* block index within a batch, or -1 */
} cda_err_info;

/* ---- context ---------------------------------------------------------- */
/* Creates a context bound to HIP device `device` (one process per GPU). */
int cda_init(int device, cda_ctx** out);
void cda_free(cda_ctx* ctx);
const char* cda_strerror(int code);
/* Last HIP error string recorded by the context (for CDA_E_DEVICE). */
const char* cda_last_device_error(cda_ctx* ctx);
/* "release gfx950", or "diagnostic gfx950 <tags>" for a library built with a diagnostic define that changes what
 * the kernels compute (timing experiments only; no environment variable can do that to a release build). */
const char* cda_build_info(void);
/* Per-context options (default 0).  CDA_OPT_HUGE_PAGES = 1: when the one-block path gets a fresh, never-touched
 * pageable EDS buffer, madvise(MADV_HUGEPAGE) its 2 MiB-aligned interior before faulting it in (faster first touch,
 * but it changes the page policy of caller memory -- under cgo, Go heap; off unless asked for).  CDA_E_ARG for an
 * unknown option. */
enum { CDA_OPT_HUGE_PAGES = 1 };
int cda_set_option(cda_ctx* ctx, int option, int64_t value);

/* ---- rsmt2d.Codec (LeoRSCodec replacement) ---------------------------- */
/* Replaces rsmt2d.LeoRSCodec selected by appconsts.DefaultCodec
 * (pkg/appconsts/global_consts.go:92).  Leopard GF(2^8) for 2k <= 256, GF(2^16) above. */
/* Codec.Encode(data [][]byte) ([][]byte, error): k data shards (contiguous,
 * k*shard_len bytes) -> k parity shards (k*shard_len). */
int cda_rs_encode(cda_ctx* ctx, uint32_t k, uint32_t shard_len, const uint8_t* data, uint8_t* parity);
/* Codec.Decode(shards [][]byte) ([][]byte, error): shards = 2k*shard_len bytes
 * (data then parity), present[i] != 0 marks available shards; missing shards are
 * reconstructed in place.  CDA_E_TOO_FEW if fewer than k are present. */
int cda_rs_decode(cda_ctx* ctx, uint32_t k, uint32_t shard_len, uint8_t* shards, const uint8_t* present);
/* Codec.MaxChunks() */
int64_t cda_rs_max_chunks(void);
/* Codec.Name() -> "Leopard" */
const char* cda_rs_name(void);
/* Codec.ValidateChunkSize(int) error */
int cda_rs_validate_chunk_size(int64_t chunk_size);

/* ---- block path: da.ExtendShares + da.NewDataAvailabilityHeader -------- */
/* Replaces da.ExtendShares (pkg/da/data_availability_header.go:65-75) followed by
 * da.NewDataAvailabilityHeader (:44-63) and DataAvailabilityHeader.Hash (:92-108).
 * shares: `count` shares of share_len bytes, row-major ODS (count must be a
 * power of two and a perfect square, k = sqrt(count)).
 * eds_or_null: 4k^2*share_len bytes row-major EDS, or NULL to skip the copy-out.
 * row_roots / col_roots: 2k*90 bytes each.  dah: 32 bytes. */
int cda_extend_commit(cda_ctx* ctx, uint32_t count, uint32_t share_len, const uint8_t* shares,
                      uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                      cda_err_info* err);

/* Batched form: nblocks independent ODS of k*k shares each, stride k*k*share_len;
 * outputs strided the same way (eds: 4k^2*share_len per block, roots 2k*90, dah 32). */
int cda_extend_commit_batch(cda_ctx* ctx, uint32_t k, uint32_t nblocks, const uint8_t* ods,
                            uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                            cda_err_info* err);

/* In-place form of cda_extend_commit for one k x k square: `eds` (4k^2*512 bytes, row-major) holds the ODS in its
 * top-left quadrant Q0 (row r of the ODS at eds + r*2k*512); the call writes Q1..Q3 around it and returns the roots
 * and DAH as cda_extend_commit.  rsmt2d's ComputeExtendedDataSquare builds the same square from the shares
 * (pkg/da/data_availability_header.go:74); go/cda's ExtendShares flattens the shares straight into Q0 of a pooled
 * page-locked EDS slab and calls this, so there is no separate share buffer and no host copy of Q0. */
int cda_extend_commit_eds(cda_ctx* ctx, uint32_t k, uint8_t* eds, uint8_t* row_roots, uint8_t* col_roots,
                          uint8_t* dah, cda_err_info* err);

/* Host buffers are streamed through the GPU in chunks: H2D of chunk i+1, the extension and trees
 * of chunk i and D2H of chunk i-1 overlap on three streams (PCIe full duplex).  Pageable memory
 * works; memory from cda_host_alloc (pinned) avoids the runtime's staging copies. */

/* Pinned host memory for share / EDS buffers (hipHostMalloc); free with cda_host_free. */
int cda_host_alloc(cda_ctx* ctx, size_t bytes, void** out);
int cda_host_free(cda_ctx* ctx, void* p);
/* Page-lock caller memory for reuse as share / EDS buffers (hipHostRegister): go/cda's buffer pools register Go-heap
 * slabs once and recycle them through the garbage collector, so the consensus path's copies are direct DMAs
 * (app/prepare_proposal.go:65, app/process_proposal.go:137, app/extend_block.go:25 through da.ExtendShares).
 * The runtime keeps the registered address after this call returns.  For Go memory that stretches cgo's rule that C
 * keeps no Go pointer: it is sound only because the gc toolchain's heap never moves an object (go/cda/pool.go states
 * the invariant; a slab is unregistered before the pool drops it and never freed while registered).  Unregister only
 * after the last call that used the range has returned (unregister first drains this context's compute, H2D, D2H
 * and auxiliary streams). */
int cda_host_register(cda_ctx* ctx, void* p, size_t bytes);
int cda_host_unregister(cda_ctx* ctx, void* p);

/* ---- multi-device batch (SURVEY.md §8b "batch ... plus a device mask", §8e) ----
 * One handle over the GPUs in `device_mask` (bit d = HIP device d; 0 = all visible devices), one
 * cda_ctx per device.  cda_multi_extend_commit_batch shards the nblocks independent blocks into
 * contiguous ranges, one per device, each streamed by its own host thread (no collective: blocks are
 * independent).  Buffers and errors as cda_extend_commit_batch; err->block is the global block index
 * of the lowest failing block. */
typedef struct cda_multi cda_multi;
int cda_multi_init(uint32_t device_mask, cda_multi** out);
void cda_multi_free(cda_multi* m);
int cda_multi_device_count(const cda_multi* m);
/* The per-device context i (0-based, in device order) for the single-device entry points. */
cda_ctx* cda_multi_context(cda_multi* m, int i);
/* HIP device id of the handle's device i (0-based, in device order), or -1. */
int cda_multi_device(const cda_multi* m, int i);
int cda_multi_extend_commit_batch(cda_multi* m, uint32_t k, uint32_t nblocks, const uint8_t* ods,
                                  uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                                  cda_err_info* err);

/* ---- one square split over the handle's devices ----
 * da.ExtendShares + NewDataAvailabilityHeader (pkg/da/data_availability_header.go:44-75) of ONE k x k square
 * (k up to 512: appconsts/testground SquareSizeUpperBound, pkg/appconsts/testground/app_consts.go:8) over the G
 * devices of `m` (G a power of two dividing k): device g row-encodes ODS rows [g k/G, (g+1) k/G), one RCCL exchange
 * (ncclSend / ncclRecv pairs in one group, communicators from ncclCommInitAll) hands every device the top half of
 * its 2k/G columns with their leaf records, each device column-encodes and roots its columns and the bottom rows'
 * subtrees over them, and device 0 folds those and hashes the DAH.  Outputs and errors as cda_extend_commit
 * (ods: k*k*512 bytes row-major; eds_or_null: 4k^2*512, gathered from the devices). */
int cda_multi_extend_commit_split(cda_multi* m, uint32_t k, const uint8_t* ods, uint8_t* eds_or_null,
                                  uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah, cda_err_info* err);
/* The same with the ODS already on the devices: d_ods_slabs[g] = device memory of device g holding ODS rows
 * [g k/G, (g+1) k/G) (k/G * k * 512 bytes).  The EDS stays on the devices (in the handle's workspace). */
int cda_multi_extend_commit_split_device(cda_multi* m, uint32_t k, const void* const* d_ods_slabs, uint8_t* row_roots,
                                         uint8_t* col_roots, uint8_t* dah, cda_err_info* err);
/* A handle of `count` contexts on ONE device whose split exchanges are device-to-device copies instead of RCCL:
 * the same plan and kernels for G = 2, 4, 8 on a single GPU (tests, rehearsal).  Free with cda_multi_free. */
int cda_multi_init_replicas(int device, uint32_t count, cda_multi** out);

/* Device-resident form (pointers are device memory of this ctx's GPU; `stream`
 * is a hipStream_t or NULL for the null stream).  Asynchronous: returns after
 * enqueueing; namespace-order errors are reported into the device word
 * `d_status` (uint64 per block: all-ones = ok, else the first namespace-order
 * violation packed as axis << 40 | axis_index << 20 | leaf) for the caller to read.
 * d_roots: nblocks * 4k * 96 bytes (row roots then col roots, 90-B node + 6 zero
 * bytes per record).  d_dah: nblocks * 32. */
int cda_extend_commit_device(cda_ctx* ctx, uint32_t k, uint32_t nblocks, const void* d_ods, void* d_eds,
                             void* d_roots, void* d_dah, void* d_status, void* stream);

/* ---- blocks of different sizes in one call (a node that replays or audits a range of heights) ----
 * Block b is a ks[b] x ks[b] square of 512-byte shares.  ks is a host array in both forms and has been read when the
 * call returns.  Every buffer is packed in block order with no padding; block b starts at
 *   ods: sum_{i<b} k_i^2 * 512      eds: sum_{i<b} 4 k_i^2 * 512      row_roots / col_roots: sum_{i<b} 2 k_i * 90
 *   dah: 32 b       d_roots: sum_{i<b} 4 k_i records of 96 B (a block's row roots, then its column roots, as
 *   cda_extend_commit_device lays them out)       d_status: one uint64 per block, encoded as there.
 * Block b comes out byte for byte as cda_extend_commit returns it for that block alone: EDS, roots and DAH.
 * Blocks with k <= CDA_OPT_MIXED_SMALL_MAX go together, whatever their sizes, into one launch of a kernel that takes
 * a square from ODS to DAH in a single workgroup.  The host form groups the other blocks by k and runs each group as
 * cda_extend_commit_batch runs a batch on the context's stream (k = 256 and 512 on GF(2^16) included).  The device
 * form gathers nothing: each maximal run of consecutive larger blocks of equal k is one pass of the
 * cda_extend_commit_device pipeline over that sub-range, so a caller who wants its large blocks fully batched
 * orders them by size.  The device form is asynchronous on `stream`, as cda_extend_commit_device is; the ODS must
 * not overlap the EDS.
 * Errors: CDA_E_ARG (a null argument, nblocks == 0); CDA_E_NOT_POW2 (some ks[b] is not a power of two; err->block =
 * the lowest such b); CDA_E_UNSUPPORTED (some ks[b] > 512; err->block = the lowest such b); CDA_E_NS_ORDER (host
 * form: err->block = the lowest failing block, axis / index / leaf what cda_extend_commit reports for that block
 * alone).
 * CDA_OPT_MIXED_SMALL_MAX (cda_set_option, per context): the largest k that goes to the one-workgroup kernel: 0
 * (none), 1, 2, 4 or 8 (the default); any other value is CDA_E_ARG.  The results are the same bytes at every value. */
int cda_extend_commit_mixed(cda_ctx* ctx, uint32_t nblocks, const uint32_t* ks, const uint8_t* ods,
                            uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                            cda_err_info* err);
int cda_extend_commit_mixed_device(cda_ctx* ctx, uint32_t nblocks, const uint32_t* ks, const void* d_ods,
                                   void* d_eds, void* d_roots, void* d_dah, void* d_status, void* stream);
enum { CDA_OPT_MIXED_SMALL_MAX = 2 }; /* cda_set_option */

/* ---- device-resident building blocks (one square split over GPUs) ----
 * All pointers are device memory of this ctx's GPU; asynchronous on `stream`
 * (hipStream_t or NULL).  They share the ctx's scratch workspace, so calls on
 * different streams of one ctx must be ordered by the caller. */

/* Batched strided Codec.Encode: for codeword c < ncw, data shard i at
 * d_src + c*src_cw + i*src_sh, parity shard i written to d_dst + c*dst_cw + i*dst_sh
 * (byte strides).  The rows of rsmt2d erasureExtendSquare are (src_cw = row
 * pitch, src_sh = shard_len), its columns (src_cw = shard_len, src_sh = row pitch). */
int cda_rs_encode_device(cda_ctx* ctx, uint32_t k, uint32_t shard_len, uint32_t ncw, const void* d_src, int64_t src_cw,
                         int64_t src_sh, void* d_dst, int64_t dst_cw, int64_t dst_sh, void* stream);

/* Erasured-NMT roots of `naxes` consecutive axes (axis = CDA_AXIS_ROW/COL,
 * indices first_index ..) of a 2k x 2k row-major EDS `d_eds` (512-B shares; only
 * the cells read are needed), over leaves [leaf_off, leaf_off + nleaves):
 * nleaves = 2k gives the axis root (eds.RowRoots / ColRoots, nmt_wrapper.go:118-124);
 * an aligned power-of-two sub-range gives the root of that subtree, which the
 * split-square path folds across GPUs.  d_roots: naxes 96-B records (90-B node +
 * 6 zero bytes).  d_status: naxes uint64, all-ones or the first leaf index whose
 * Push order check failed (nmt ErrInvalidPushOrder). */
int cda_nmt_roots_device(cda_ctx* ctx, uint32_t k, const void* d_eds, uint32_t axis, uint32_t first_index,
                         uint32_t naxes, uint32_t leaf_off, uint32_t nleaves, void* d_roots, void* d_status,
                         void* stream);

/* ntrees x n (power of two) contiguous 96-B node records -> ntrees root records
 * (NmtHasher.HashNode levels, test/util/malicious/hasher.go:271-310). */
int cda_nmt_fold_device(cda_ctx* ctx, uint32_t ntrees, uint32_t n, const void* d_nodes, void* d_roots, void* stream);

/* DataAvailabilityHeader.Hash over n_total 96-B root records (row roots then
 * column roots) -> 32 B (pkg/da/data_availability_header.go:92-108). */
int cda_dah_device(cda_ctx* ctx, uint32_t n_total, const void* d_roots, void* d_dah, void* stream);

/* Roots + DAH of an existing EDS (rsmt2d eds.RowRoots/ColRoots + DAH hash). */
int cda_commit_eds(cda_ctx* ctx, uint32_t k, const uint8_t* eds, uint8_t* row_roots, uint8_t* col_roots,
                   uint8_t* dah, cda_err_info* err);

/* DataAvailabilityHeader.Hash() over given roots (RFC-6962, go-square/merkle
 * HashFromByteSlices over rowRoots ‖ colRoots; n roots per axis, 90 B each). */
int cda_dah_hash(cda_ctx* ctx, uint32_t n, const uint8_t* row_roots, const uint8_t* col_roots, uint8_t* dah);

/* ---- wrapper.NewConstructor tree (rsmt2d.TreeConstructorFn) ------------ */
/* Root of one erasured NMT axis: replaces ErasuredNamespacedMerkleTree
 * Push x n + Root (pkg/wrapper/nmt_wrapper.go:93-124) for square size k and
 * axis index `axis_index`.  leaves: n * leaf_len bytes. */
int cda_nmt_axis_root(cda_ctx* ctx, uint64_t square_size, uint64_t axis_index, uint32_t n, uint32_t leaf_len,
                      const uint8_t* leaves, uint8_t* root, cda_err_info* err);

/* ---- rsmt2d Repair ------------------------------------------------------ */
/* Replaces (*rsmt2d.ExtendedDataSquare).Repair(rowRoots, colRoots): eds is the
 * 4k^2*share_len square with missing cells marked by present[r*2k+c] == 0;
 * repaired in place (present updated).  Returns CDA_OK, CDA_E_UNREPAIRABLE or
 * CDA_E_BYZANTINE (err->axis/index). */
int cda_repair(cda_ctx* ctx, uint32_t k, uint8_t* eds, uint8_t* present, const uint8_t* row_roots,
               const uint8_t* col_roots, cda_err_info* err);
/* The same on a square already in device memory of this ctx's GPU (d_eds, 4k^2*512 bytes, repaired
 * in place; e.g. assembled there from proved samples by cda_samples_assemble_device, or the output of
 * cda_extend_commit_device).  present / roots / err are host memory.  Ordered after prior work on
 * `stream` (0 = the null stream); returns when the repair is complete. */
int cda_repair_device(cda_ctx* ctx, uint32_t k, void* d_eds, uint8_t* present, const uint8_t* row_roots,
                      const uint8_t* col_roots, cda_err_info* err, void* stream);

/* ---- blob share commitments (x/blob, go-square inclusion) -------------- */
/* inclusion.CreateCommitments(blobs, merkle.HashFromByteSlices, threshold)
 * (x/blob/types/payforblob.go:53; CreateCommitment per blob in ValidateBlobTx,
 * blob_tx.go:97-105).  Blob b = namespace namespaces[29b, 29b+29) and data
 * data[offsets[b], offsets[b+1]); share_versions may be NULL (all 0).
 * commitments: nblobs x 32 B.  Errors name the blob in err->index, checked in
 * ValidateBlobs' order (payforblob.go:230-236): CDA_E_BLOB_SIZE, CDA_E_SHARE_VERSION. */
int cda_blob_commitments(cda_ctx* ctx, uint32_t nblobs, const uint8_t* namespaces, const uint8_t* data,
                         const uint64_t* offsets, const uint8_t* share_versions, uint32_t subtree_root_threshold,
                         uint8_t* commitments, cda_err_info* err);

/* merkle.HashFromByteSlices over sets of 90-B NMT nodes (the subtree-root fold of
 * pkg/inclusion/get_commit.go:29): set s = items[off[s]-off[0], off[s+1]-off[0]);
 * roots: nsets x 32 B; an empty set hashes to SHA256("").  item_len must be 90. */
int cda_merkle_roots(cda_ctx* ctx, uint32_t nsets, const uint32_t* set_offsets, const uint8_t* items,
                     uint32_t item_len, uint8_t* roots);

/* ---- NMT node export and share inclusion proofs (pkg/inclusion, pkg/proof) ---- */
/* cda_extend_commit plus every node of the trees the block path builds: what the
 * inner-node cache of pkg/inclusion/nmt_caching.go:76-124 records through nmt's
 * NodeVisitor, and what pkg/proof/proof.go:82-153 recomputes for proofs.
 * row_nodes / col_nodes (optional): 2k trees x (4k-1) nodes x 90 B; per tree the
 * 2k leaves first, then each level, the root last.  dah_nodes (optional):
 * (8k-1) x 32 B, the RFC-6962 tree over rowRoots ‖ colRoots, leaf hashes first,
 * the data root last. */
int cda_extend_commit_nodes(cda_ctx* ctx, uint32_t count, uint32_t share_len, const uint8_t* shares,
                            uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah,
                            uint8_t* row_nodes, uint8_t* col_nodes, uint8_t* dah_nodes, cda_err_info* err);

typedef struct {
  uint32_t start_row, end_row; /* RowProof.StartRow / EndRow */
  uint32_t nrows;              /* end_row - start_row + 1 */
  uint32_t total;              /* Proof.Total = 4k (rowRoots ‖ colRoots) */
  uint32_t naunts;             /* aunts per row proof = log2(4k) */
  uint32_t max_nodes;          /* node slots per row in nmt_nodes = 2 log2(2k) */
} cda_share_proof_info;

/* pkg/proof NewShareInclusionProof (proof.go:55-167) for the ODS shares
 * [start, end) of the k x k square `shares` (count = k*k).  Per proven row i
 * (capacity k rows): row_roots 90 B; the row root's RFC-6962 proof in the data
 * root (merkle.ProofsFromByteSlices, :82-93): leaf_hashes 32 B, aunts naunts x 32 B
 * bottom-up; the NMT range proof (ProveRange, :129-152): nmt_start / nmt_end /
 * nmt_count and nmt_nodes (max_nodes x 90-B slots, left to right).  data_root
 * (optional): the DAH hash.  ShareProof.Data is the caller's input range. */
int cda_share_inclusion_proof(cda_ctx* ctx, uint32_t count, uint32_t share_len, const uint8_t* shares, uint32_t start,
                              uint32_t end, cda_share_proof_info* info, uint8_t* row_roots, uint8_t* leaf_hashes,
                              uint8_t* aunts, int32_t* nmt_start, int32_t* nmt_end, int32_t* nmt_count,
                              uint8_t* nmt_nodes, uint8_t* data_root, cda_err_info* err);

/* ---- sample proofs: prove any EDS cell, verify proved cells in batches ---- */
/* A retained square: the block is extended once and the EDS with every node of its 4k trees stays in
 * device memory that belongs to the handle (never the context's workspace: other calls on the context
 * leave it untouched), and with them the RFC-6962 tree over rowRoots ‖ colRoots (8k - 1 nodes of 32 B, the layout of
 * cda_extend_commit_nodes' dah_nodes) that cda_square_share_proofs reads leaf hashes and aunts from.  Calls on a handle take its context's lock.  cda_free of a context with open
 * squares releases their device memory; such a handle stays valid for cda_square_close only (every
 * other call on it returns CDA_E_ARG), so close after free never touches the device. */
typedef struct cda_square cda_square;
/* da.ExtendShares + NewDataAvailabilityHeader as cda_extend_commit (same outputs, same
 * CDA_E_NS_ORDER mapping, on which no handle is returned); *out receives the handle. */
int cda_square_open(cda_ctx* ctx, uint32_t count, uint32_t share_len, const uint8_t* shares, cda_square** out,
                    uint8_t* row_roots, uint8_t* col_roots, uint8_t* dah, cda_err_info* err);
/* Retains a square as it was committed: eds is the whole extended square, (2k)^2 x 512 B row-major in host memory,
 * k a power of two.  Nothing is extended and the encoding is NOT checked: the handle commits to whatever it was given
 * (a downloaded or repaired EDS, or a badly encoded one whose cells a bad-encoding fraud proof must carry).  Outputs,
 * CDA_E_NS_ORDER mapping and every call on the handle as for cda_square_open. */
int cda_square_open_eds(cda_ctx* ctx, uint32_t k, const uint8_t* eds, cda_square** out, uint8_t* row_roots,
                        uint8_t* col_roots, uint8_t* dah, cda_err_info* err);
void cda_square_close(cda_square* sq);

typedef struct {
  uint32_t axis, index; /* CDA_AXIS_ROW / CDA_AXIS_COL, 0 <= index < 2k: the tree */
  uint32_t start, end;  /* wrapper ErasuredNamespacedMerkleTree.ProveRange(start, end), 0 <= start < end <= 2k */
} cda_range_query;
/* nq range proofs in one launch (wrapper.ProveRange, pkg/wrapper/nmt_wrapper.go:127-130, of any row or
 * column tree, parity cells included).  counts[q] = proof nodes of query q; nodes: nq x max_nodes slots
 * of 90 B, a query's nodes left to right in its first counts[q] slots (the others zero);
 * max_nodes >= 2 log2(2k), else CDA_E_ARG.  shares_or_null receives the proved cells packed in query
 * order, sum(end - start) x 512 B; shares_cap is its size in bytes (CDA_E_ARG if too small).  A query
 * outside the square gives CDA_E_ARG before anything is launched.  q is host memory; counts, nodes and
 * shares_or_null may each be host or device memory. */
int cda_square_prove(cda_square* sq, uint32_t nq, const cda_range_query* q, uint32_t max_nodes, int32_t* counts,
                     uint8_t* nodes, uint8_t* shares_or_null, uint64_t shares_cap);

/* Batched nmt.Proof.VerifyInclusion (IgnoreMaxNamespace, as ShareProof.VerifyProof calls it).  Proof p:
 * namespace = namespaces[29p, 29p + 29), leaves = leaves[leaf_off, leaf_off + end - start) (512-B shares
 * without the namespace prefix: a leaf hashes as ns ‖ ns ‖ SHA256(0x00 ‖ ns ‖ share) with the supplied
 * namespace), nodes = nodes[node_off, node_off + nnodes) of 90 B, root = roots[root] of 90 B. */
typedef struct {
  uint32_t start, end, node_off, nnodes, leaf_off, root;
} cda_nmt_proof_desc;
/* ok[p] = 1 if proof p verifies, else 0: a false proof is a verdict, never an error code.  A descriptor
 * that points outside the totals or has start >= end gets 0 and is not read through.  CDA_E_ARG if a
 * descriptor has end > 65536 (the widest axis the codec accepts). */
int cda_nmt_verify(cda_ctx* ctx, uint32_t nproofs, const cda_nmt_proof_desc* descs, const uint8_t* namespaces,
                   const uint8_t* roots, uint32_t nroots, const uint8_t* nodes, uint32_t nnodes_total,
                   const uint8_t* leaves, uint32_t nleaves_total, uint8_t* ok);
/* The same with every pointer in device memory (d_leaves 16-byte, d_nodes / d_roots / d_descs 4-byte
 * aligned, else CDA_E_ARG), asynchronous on `stream`; a descriptor with end > 65536 gets ok = 0. */
int cda_nmt_verify_device(cda_ctx* ctx, uint32_t nproofs, const void* d_descs, const void* d_namespaces,
                          const void* d_roots, uint32_t nroots, const void* d_nodes, uint32_t nnodes_total,
                          const void* d_leaves, uint32_t nleaves_total, void* d_ok, void* stream);

/* ---- share proofs to the data root: many per launch from a retained square, batched Validate ---- */
/* ODS shares [start, end), row-major, 0 <= start < end <= k*k: the range ParseNamespace has validated
 * (pkg/proof/querier.go:126-158). */
typedef struct {
  uint32_t start, end;
} cda_share_range;
/* One row of a ShareProof: the NMTProof of the row's shares (ShareProof.ShareProofs[i]) and the merkle Proof of
 * the row root in the data root (RowProof.Proofs[i]).  Row record r goes with row_roots[r] (90 B, RowProof.RowRoots)
 * and leaf_hashes[r] (32 B, Proof.LeafHash); its nodes and aunts are addressed in the flat arrays. */
typedef struct {
  int32_t nmt_start, nmt_end; /* NMTProof.Start / End (signed, as in proof.pb.go) */
  uint32_t node_off, nnodes;  /* NMTProof.Nodes = nodes[node_off, node_off + nnodes) of 90 B */
  int64_t total, index;       /* Proof.Total / Index */
  uint32_t aunt_off, naunts;  /* Proof.Aunts = aunts[aunt_off, aunt_off + naunts) of 32 B, bottom-up */
  uint32_t row;               /* the row of the square (cda_square_share_proofs; cda_share_proofs_validate ignores it) */
  uint32_t pad_;
} cda_share_row;
/* pkg/proof NewShareInclusionProof (proof.go:55-167) for nq ranges of a retained square in one launch: nothing is
 * extended or hashed again.  Query q proves rows start / k .. (end - 1) / k (proof.go:61-64); its row records are
 * rows[row_off[q], row_off[q + 1]) (row_off: nq + 1 words).  Per row the NMT range is [start % k, k) on the first
 * row, [0, k) between, [0, (end - 1) % k + 1) on the last (proof.go:129-139); record r has node_off = r * max_nodes
 * (the slots after its nnodes nodes are zero), aunt_off = r * log2(4k), naunts = log2(4k), total = 4k, index = row
 * (merkle.ProofsFromByteSlices over rowRoots ‖ colRoots, proof.go:82-93).  Capacities: rows_cap row records in rows /
 * nodes (x max_nodes x 90 B) / row_roots (x 90) / leaf_hashes (x 32) / aunts (x log2(4k) x 32); shares_cap bytes in
 * shares_or_null, which receives the proved shares (ShareProof.Data) packed in query order.  data_root: 32 B, once.
 * CDA_E_ARG before any launch for a range outside the square, max_nodes < 2 log2(2k) or a capacity too small.
 * q is host memory; every output may be host or device memory. */
int cda_square_share_proofs(cda_square* sq, uint32_t nq, const cda_share_range* q, uint32_t max_nodes,
                            uint32_t rows_cap, uint32_t* row_off, cda_share_row* rows, uint8_t* nodes,
                            uint8_t* row_roots, uint8_t* leaf_hashes, uint8_t* aunts, uint8_t* shares_or_null,
                            uint64_t shares_cap, uint8_t* data_root);

/* One ShareProof of a cda_share_proofs_validate batch over flat arrays: ShareProofs / RowRoots / Proofs are the first
 * nshare_proofs / nrow_roots / nrow_proofs of the row records from row_off (a well-formed proof has the three equal),
 * Data = leaves[leaf_off, leaf_off + nleaves) of 512 B, the root to validate against = data_roots[data_root]. */
typedef struct {
  uint32_t row_off;
  uint32_t nshare_proofs, nrow_roots, nrow_proofs;
  uint32_t leaf_off, nleaves;
  uint32_t start_row, end_row; /* RowProof.StartRow / EndRow */
  uint32_t data_root;
  uint8_t ns[29]; /* NamespaceVersion ‖ NamespaceID */
  uint8_t pad_[3];
} cda_share_proof_desc;
/* Verdicts: 0, or the first check of ShareProof.Validate that fails, in its order (share_proof.go:16-51,
 * RowProof.Validate row_proof.go:13-24). */
enum {
  CDA_SP_VALID = 0,
  CDA_SP_PROOF_COUNT = 1, /* "the number of share proofs ... must equal the number of row roots" */
  CDA_SP_DATA_COUNT = 2,  /* "the number of shares ... must equal the number of shares in share proofs" */
  CDA_SP_NEG_START = 3,   /* "proof index cannot be negative" */
  CDA_SP_EMPTY_RANGE = 4, /* "proof total must be positive" */
  CDA_SP_ROW_COUNT = 5,   /* "the number of rows ... must equal the number of row roots" */
  CDA_SP_ROW_PROOFS = 6,  /* "the number of proofs ... must equal the number of row roots" */
  CDA_SP_ROW_PROOF = 7,   /* "row proof failed to verify" (merkle Proof.Verify of a row root, row_proof.go:26-48) */
  CDA_SP_SHARE_PROOF = 8, /* "share proof failed to verify" (nmt VerifyInclusion of a row, share_proof.go:53-82) */
  CDA_SP_MALFORMED = 9,   /* a descriptor points outside the totals, or shares row records with another proof:
                             nothing is read through it */
};
/* Batched ShareProof.Validate: verdicts[p] (int32) for proof p.  A false proof is a verdict, never an error code.
 * The arrays cda_square_share_proofs writes are accepted as they lie.  nrows / nnodes / naunts / nleaves / nroots
 * are the totals of rows (and row_roots, leaf_hashes) / nodes / aunts / leaves / data_roots. */
int cda_share_proofs_validate(cda_ctx* ctx, uint32_t nproofs, const cda_share_proof_desc* descs,
                              const cda_share_row* rows, const uint8_t* row_roots, const uint8_t* leaf_hashes,
                              uint32_t nrows, const uint8_t* nodes, uint32_t nnodes, const uint8_t* aunts,
                              uint32_t naunts, const uint8_t* leaves, uint32_t nleaves, const uint8_t* data_roots,
                              uint32_t nroots, int32_t* verdicts);
/* The same with every pointer in device memory (d_leaves 16-byte, d_rows 8-byte, the others 4-byte aligned, else
 * CDA_E_ARG), asynchronous on `stream`; every check is made in the kernels.  Uses the context's workspace. */
int cda_share_proofs_validate_device(cda_ctx* ctx, uint32_t nproofs, const void* d_descs, const void* d_rows,
                                     const void* d_row_roots, const void* d_leaf_hashes, uint32_t nrows,
                                     const void* d_nodes, uint32_t nnodes, const void* d_aunts, uint32_t naunts,
                                     const void* d_leaves, uint32_t nleaves, const void* d_data_roots,
                                     uint32_t nroots, void* d_verdicts, void* stream);

/* ---- blob commitment proofs: "the blob with share commitment C is in the block with data root R", without the
 * blob's shares (ADR-011 "Blob Inclusion Proof"): the blob's subtree roots, their proofs to the row roots and on to
 * the data root, and the commitment over the subtree roots.  Parity unpinned: the verifier's rule list C0-C8 is this
 * project's statement; its counterpart lives in celestia-node and nmt, outside the reference tree. ---- */
/* ODS shares [start, start + len), row-major: a blob as square.Construct placed it (start a multiple of its
 * SubTreeWidth). */
typedef struct {
  uint32_t start, len;
} cda_blob_range;
/* One row of a commitment proof.  Row record r goes with row_roots[r] (90 B) and leaf_hashes[r] (32 B), as a
 * cda_share_row does. */
typedef struct {
  int32_t nmt_start, nmt_end; /* the row's leaf range, as cda_share_row */
  uint32_t node_off, nnodes;  /* ProveRange(nmt_start, nmt_end) of the row tree = nodes[node_off, +nnodes) of 90 B */
  uint32_t root_off, nroots;  /* the range's subtree roots = subtree_roots[root_off, +nroots) of 90 B, left to right */
  int64_t total, index;       /* Proof.Total / Index of the row root in the data root: 4k, row */
  uint32_t aunt_off, naunts;  /* Proof.Aunts = aunts[aunt_off, +naunts) of 32 B, bottom-up */
  uint32_t row;               /* the row of the square (the prover's; the verifier ignores it) */
  uint32_t pad_;
} cda_commitment_row;
/* The row records and subtree roots cda_square_commitment_proofs writes for nq ranges of a k x k square under
 * subtree_root_threshold.  CDA_E_ARG for what that call rejects in a range (below), CDA_E_NOT_POW2 for k. */
int cda_commitment_proof_sizes(uint32_t k, uint32_t subtree_root_threshold, uint32_t nq, const cda_blob_range* q,
                               uint64_t* nrows, uint64_t* nroots);
/* Commitment proofs of nq blobs of a retained square in one call: nothing is extended or hashed again but the
 * commitments.  Blob q has W = SubTreeWidth(len, subtree_root_threshold) and rows start / k .. (start + len - 1) / k;
 * its row records are rows[row_off[q], row_off[q + 1]) (row_off: nq + 1 words) and its subtree roots lie contiguous in
 * subtree_roots, row after row, left to right (pkg/inclusion/paths.go's coordinates).  Record r has node_off =
 * r * max_nodes (the slots after its nnodes nodes are zero), aunt_off = r * log2(4k), naunts = log2(4k), total = 4k,
 * index = row.  commitments[q] (32 B) = merkle.HashFromByteSlices over blob q's subtree roots = GetCommitment
 * (pkg/inclusion/get_commit.go).  Capacities: rows_cap row records in rows / nodes (x max_nodes x 90 B) / row_roots
 * (x 90) / leaf_hashes (x 32) / aunts (x log2(4k) x 32); roots_cap subtree roots of 90 B.  data_root: 32 B, once.
 * Commitments only: row_off, rows, nodes, subtree_roots, row_roots, leaf_hashes, aunts and data_root all NULL (the
 * capacities are then ignored).  CDA_E_ARG before any launch for len == 0, a range outside the ODS, threshold == 0,
 * W > k, start % W != 0, max_nodes < 2 log2(2k) or a capacity too small; CDA_E_UNSUPPORTED for a blob of more than
 * 262,144 subtree roots.  q is host memory; every output may be host or device memory. */
int cda_square_commitment_proofs(cda_square* sq, uint32_t nq, const cda_blob_range* q,
                                 uint32_t subtree_root_threshold, uint32_t max_nodes, uint32_t rows_cap,
                                 uint32_t roots_cap, uint32_t* row_off, cda_commitment_row* rows, uint8_t* nodes,
                                 uint8_t* subtree_roots, uint8_t* row_roots, uint8_t* leaf_hashes, uint8_t* aunts,
                                 uint8_t* commitments, uint8_t* data_root);

/* One commitment proof of a cda_commitment_proofs_verify batch over flat arrays: its rows are the row records
 * [row_off, row_off + nrows); it is verified against data_roots[data_root] and commitments[commitment]. */
typedef struct {
  uint32_t row_off, nrows;
  uint32_t start_row, end_row;
  uint32_t data_root, commitment;
  uint32_t subtree_root_threshold;
  uint8_t ns[29]; /* the blob's namespace: NamespaceVersion ‖ NamespaceID */
  uint8_t pad_[3];
} cda_commitment_proof_desc;
/* Verdicts: 0, or the first rule that fails, in this order. */
enum {
  CDA_CP_VALID = 0,
  CDA_CP_MALFORMED = 1,     /* C0: offsets or counts outside the totals, nrows == 0, threshold == 0, more than 262,144
                               subtree roots, or row records shared with another proof: nothing is read through it */
  CDA_CP_ROW_COUNT = 2,     /* C1: end_row - start_row + 1 != nrows */
  CDA_CP_RANGE = 3,         /* C2: the rows' ranges are not one contiguous range of a k x k ODS (total = 4k, index =
                               start_row + i, 0 <= nmt_start < nmt_end <= k, inner edges at 0 and k) */
  CDA_CP_ALIGNMENT = 4,     /* C3: W = SubTreeWidth(sum of the ranges, threshold) > k, or the first nmt_start % W != 0 */
  CDA_CP_ROOT_COUNT = 5,    /* C4: a row's nroots is not the number of tiles of its range under W */
  CDA_CP_NAMESPACE = 6,     /* C5: a subtree root whose min or max namespace is not ns */
  CDA_CP_ROW_PROOF = 7,     /* C6: merkle Proof.Verify of a row root in the data root fails */
  CDA_CP_SUBTREE_ROOTS = 8, /* C7: a row's subtree roots and nodes do not fold to its row root (wrong node count or
                               sibling order included) */
  CDA_CP_COMMITMENT = 9,    /* C8: the RFC-6962 root over all subtree roots, in order, is not the commitment */
};
/* Batched verification: verdicts[p] (int32) for proof p.  A false proof is a verdict, never an error code.  The arrays
 * cda_square_commitment_proofs writes are accepted as they lie.  nrows / nnodes / nsubtree_roots / naunts / nroots /
 * ncommitments are the totals of rows (and row_roots, leaf_hashes) / nodes / subtree_roots / aunts / data_roots /
 * commitments. */
int cda_commitment_proofs_verify(cda_ctx* ctx, uint32_t nproofs, const cda_commitment_proof_desc* descs,
                                 const cda_commitment_row* rows, const uint8_t* row_roots, const uint8_t* leaf_hashes,
                                 uint32_t nrows, const uint8_t* nodes, uint32_t nnodes, const uint8_t* subtree_roots,
                                 uint32_t nsubtree_roots, const uint8_t* aunts, uint32_t naunts,
                                 const uint8_t* data_roots, uint32_t nroots, const uint8_t* commitments,
                                 uint32_t ncommitments, int32_t* verdicts);
/* The same with every pointer in device memory (d_rows 8-byte, the others 4-byte aligned, else CDA_E_ARG),
 * asynchronous on `stream`; every check is made in the kernels.  Uses the context's workspace. */
int cda_commitment_proofs_verify_device(cda_ctx* ctx, uint32_t nproofs, const void* d_descs, const void* d_rows,
                                        const void* d_row_roots, const void* d_leaf_hashes, uint32_t nrows,
                                        const void* d_nodes, uint32_t nnodes, const void* d_subtree_roots,
                                        uint32_t nsubtree_roots, const void* d_aunts, uint32_t naunts,
                                        const void* d_data_roots, uint32_t nroots, const void* d_commitments,
                                        uint32_t ncommitments, void* d_verdicts, void* stream);

/* ---- what is in a retained square: its sequences (the two compact ones and the blobs) read back from the shares,
 * the blobs' share commitments, and the payload bytes with the share headers stripped (celestia-node's
 * blob.Get / GetAll / GetProof / Included start here).  Parity unpinned: go-square's shares package is not in the
 * reference tree; the rule (csrc/share_index_rule.h) restates specs/src/specs/shares.md and namespace.md. ---- */
enum { CDA_SEQ_KIND_TX = 0, CDA_SEQ_KIND_PFB = 1, CDA_SEQ_KIND_BLOB = 2 };
/* Status of a sequence: a bit mask, every bit that applies.  A hostile square gives statuses, never an error code. */
enum {
  CDA_SEQ_TRUNCATED = 1,   /* start + nshares > k^2 */
  CDA_SEQ_BROKEN = 2,      /* inside its claim: another start share (padding or not), or a continuation share of
                              another namespace or share version */
  CDA_SEQ_VERSION = 4,     /* share version != 0 */
  CDA_SEQ_RESERVED_NS = 8, /* a blob in a primary (version 0, id <= 255) or secondary (version 255) reserved namespace */
  CDA_SEQ_UNALIGNED = 16,  /* a blob with W = SubTreeWidth(nshares, threshold) > k or start % W != 0: no commitment
                              exists for it in this square (not looked at when the threshold is 0) */
};
typedef struct {
  uint32_t start, nshares; /* claimed extent [start, start + nshares) of the ODS, row-major */
  uint32_t seq_len;        /* payload bytes */
  uint8_t kind, share_version, status, pad_;
  uint8_t ns[29];
  uint8_t pad2_[3];
} cda_sequence; /* 48 B */
typedef struct {
  uint32_t k, nseq, npadding, norphans, first_orphan; /* first_orphan 0xFFFFFFFF: none */
} cda_square_summary;
#ifdef __cplusplus
static_assert(sizeof(cda_sequence) == 48 && sizeof(cda_square_summary) == 20, "record sizes are part of the ABI");
#else
_Static_assert(sizeof(cda_sequence) == 48 && sizeof(cda_square_summary) == 20, "record sizes are part of the ABI");
#endif
/* Every sequence of a retained square in ascending order, and (commitments != NULL) the share commitment of every
 * blob whose status is 0 under subtree_root_threshold, from the retained tree nodes (GetCommitment); every other
 * record's commitment is 32 zero bytes.  Writes min(nseq, cap) records (and commitments); summary->nseq is the count.
 * An orphan is a continuation share with no start share before it, after a padding share or past its sequence's claim:
 * counted, the first one reported, part of no sequence.  seqs and commitments may be host or device memory (seqs may be
 * NULL when cap is 0); summary is host memory.  seqs and commitments are written after the commitments were computed
 * and summary last, on success only: a call that fails there or earlier leaves all three as they were.  CDA_E_ARG
 * before any launch for a null handle or summary, or subtree_root_threshold == 0 when commitments are asked for. */
int cda_square_index(cda_square* sq, uint32_t subtree_root_threshold, uint32_t cap, cda_sequence* seqs,
                     uint8_t* commitments, cda_square_summary* summary);
typedef struct {
  uint32_t start, nshares, seq_len, compact; /* a cda_sequence's extent and length; compact: kind is TX or PFB */
} cda_sequence_range;
/* Payloads of nq sequences, headers stripped (34 B of a blob's first share and 30 B of its later ones; 38 B and 34 B of
 * a compact sequence's), query q at data[data_off[q], + seq_len).  No byte outside those ranges is written;
 * overlapping ranges are the caller's business.  q and data_off are host memory, data host or device memory.
 * CDA_E_ARG before any launch for a null handle, start + nshares > k^2, nshares smaller than seq_len needs, or
 * data_off[q] + seq_len > data_cap. */
int cda_square_read(cda_square* sq, uint32_t nq, const cda_sequence_range* q, const uint64_t* data_off,
                    uint64_t data_cap, uint8_t* data);

/* ---- namespace data with completeness proofs: nmt ProveNamespace / Proof.VerifyNamespace, batched ---- */
/* "Everything of namespace ns in tree (axis, index), and a proof that nothing was withheld."  Namespaces compare as
 * 29-byte big-endian strings; leaf i's namespace is the share's own in Q0 and 0xFF x 29 elsewhere. */
typedef struct {
  uint32_t axis, index;
  uint8_t ns[29];
  uint8_t pad_[3];
} cda_namespace_query;
enum { CDA_NSP_EMPTY = 0, CDA_NSP_INCLUSION = 1, CDA_NSP_ABSENCE = 2 };
/* EMPTY (ns outside the root's [min, max]): start = end = 0, no nodes.  INCLUSION: [start, end) is the namespace's
 * run of leaves, nodes = ProveRange(start, end), the run's cells are shares[share_off, share_off + nshares).
 * ABSENCE (inside the root's range, not present): [start, start + 1) is the first leaf with a larger namespace, nodes
 * = ProveRange(start, start + 1), leaf_hashes[q] is that leaf's 90-B node (NMTProof.leaf_hash), no shares. */
typedef struct {
  uint32_t kind, start, end, nnodes, share_off, nshares;
} cda_namespace_result;
/* nq queries of a retained square in one call.  results: nq records; nodes: nq x max_nodes x 90 B (query q's from
 * slot q * max_nodes, unused slots zero); leaf_hashes: nq x 90 B (zero unless ABSENCE); shares_or_null: the shares of
 * the INCLUSION results packed in query order, share_off[q] = the shares of the queries before q.  The share count
 * depends on the data: *nshares_total (host memory) is always written; if shares_or_null is non-null and shares_cap
 * (bytes) is too small the shares are not written, everything else is, and the call returns CDA_E_ARG (nq x 2k x 512
 * bytes always suffice).  CDA_E_ARG before any launch for axis > 1, index >= 2k, max_nodes < 2 log2(2k) or a
 * detached handle.  q is host memory; results, nodes, leaf_hashes and shares_or_null may each be host or device
 * memory. */
int cda_square_prove_namespace(cda_square* sq, uint32_t nq, const cda_namespace_query* q, uint32_t max_nodes,
                               cda_namespace_result* results, uint8_t* nodes, uint8_t* leaf_hashes,
                               uint8_t* shares_or_null, uint64_t shares_cap, uint64_t* nshares_total);

#define CDA_NO_LEAF_HASH 0xFFFFFFFFu
/* One proof of a cda_nmt_verify_namespace batch: nodes = nodes[node_off, node_off + nnodes) of 90 B, leaves =
 * leaves[leaf_off, leaf_off + nleaves) of 512 B, root = roots[root] of 90 B, leaf_hash = leaf_hashes[leaf_hash] of
 * 90 B or CDA_NO_LEAF_HASH; the namespace is namespaces[29p, 29p + 29). */
typedef struct {
  uint32_t start, end, node_off, nnodes, leaf_off, nleaves, root, leaf_hash;
} cda_nmt_ns_proof_desc;
/* Batched nmt Proof.VerifyNamespace (IgnoreMaxNamespace): ok[p] = 1 iff
 *   - root, every node and the leaf hash have min <= max;
 *   - start == end: no nodes, no leaf hash, no leaves, and ns outside the root's [min, max] or the root is that of the
 *     empty tree; start > end is false;
 *   - with a leaf hash (absence; leaves are ignored): end == start + 1 and ns < leaf_hash.min, and the root is
 *     recomputed from the leaf hash as leaf `start`;
 *   - without one (inclusion): nleaves == end - start, leaves hashed under the supplied namespace as cda_nmt_verify;
 *   - completeness: the first popcount(start) nodes have max < ns, every later node has min > ns;
 *   - the recomputed root (cda_nmt_verify's rules) equals the root.
 * A false proof is a verdict, never an error code.  A descriptor outside the totals gets 0 and is not read through.
 * The arrays cda_square_prove_namespace writes are accepted as they lie (node_off = q x max_nodes, leaf_hash = q for
 * ABSENCE, leaf_off = share_off).  CDA_E_ARG if a descriptor has end > 65536. */
int cda_nmt_verify_namespace(cda_ctx* ctx, uint32_t nproofs, const cda_nmt_ns_proof_desc* descs,
                             const uint8_t* namespaces, const uint8_t* roots, uint32_t nroots, const uint8_t* nodes,
                             uint32_t nnodes_total, const uint8_t* leaf_hashes, uint32_t nleaf_hashes,
                             const uint8_t* leaves, uint32_t nleaves_total, uint8_t* ok);
/* The same with every pointer in device memory (d_leaves 16-byte, d_nodes / d_roots / d_leaf_hashes / d_descs 4-byte
 * aligned, else CDA_E_ARG), asynchronous on `stream`; a descriptor with end > 65536 gets ok = 0.  Uses the context's
 * workspace. */
int cda_nmt_verify_namespace_device(cda_ctx* ctx, uint32_t nproofs, const void* d_descs, const void* d_namespaces,
                                    const void* d_roots, uint32_t nroots, const void* d_nodes, uint32_t nnodes_total,
                                    const void* d_leaf_hashes, uint32_t nleaf_hashes, const void* d_leaves,
                                    uint32_t nleaves_total, void* d_ok, void* stream);

/* ---- bad-encoding fraud proofs: batched Validate (specs fraud_proofs.md, rsmt2d ErrByzantineData) ---- */
/* One proof: axis (axis, index) of a 2k x 2k square, nshares of its cells as entries[entry_off, entry_off + nshares)
 * in strictly increasing position, each proved against the ORTHOGONAL root; the block's roots are
 * roots[root_off, root_off + 4k) of 90 B, the 2k row roots then the 2k column roots. */
typedef struct {
  uint32_t axis, index, entry_off, nshares, root_off;
} cda_befp_desc;
/* Entry e: cell `pos` of the axis, its share shares[512 e, 512 e + 512), the nodes of its proof of leaf
 * [index, index + 1) in the orthogonal tree nodes[node_off, node_off + nnodes) of 90 B. */
typedef struct {
  uint32_t pos, node_off, nnodes;
} cda_befp_entry;
#define CDA_BEFP_FRAUD 1       /* the proof holds: the committed axis is not the encoding of its shares */
#define CDA_BEFP_NO_FRAUD 0    /* the shares rebuild the committed axis root */
#define CDA_BEFP_MALFORMED -1  /* axis > 1, index >= 2k, nshares > 2k, a position >= 2k or not increasing, or a
                                  descriptor or entry outside the totals: nothing is read through it */
#define CDA_BEFP_TOO_FEW -2    /* fewer than k shares */
#define CDA_BEFP_BAD_SHARE -3  /* a share fails VerifyInclusion against its orthogonal root */
/* Batched Validate, the first check that applies deciding: MALFORMED, TOO_FEW, BAD_SHARE (the namespace of a share is
 * its own first 29 bytes if index < k and pos < k, else 0xFF x 29), then the shares are put into 2k slots, the axis
 * decoded, slots [k, 2k) replaced by the encoding of slots [0, k) and the wrapper tree (squareSize k, axisIndex index)
 * built: FRAUD if it cannot be built (push order) or its root differs from the committed root of the axis, else
 * NO_FRAUD.  verdicts[p] (int32); a false proof is a verdict, never an error code.  All proofs of a call share k (a
 * power of two, else CDA_E_ARG; k <= 512, else CDA_E_UNSUPPORTED); they may belong to different blocks through
 * root_off.  nentries / nnodes_total / nroots are the totals of entries (and shares) / nodes / roots. */
int cda_befp_validate(cda_ctx* ctx, uint32_t k, uint32_t nproofs, const cda_befp_desc* descs,
                      const cda_befp_entry* entries, uint32_t nentries, const uint8_t* shares, const uint8_t* nodes,
                      uint32_t nnodes_total, const uint8_t* roots, uint32_t nroots, int32_t* verdicts);
/* The same with every pointer in device memory (d_shares 16-byte, the others 4-byte aligned, else CDA_E_ARG),
 * asynchronous on `stream`; every check is made in the kernels.  Uses the context's workspace. */
int cda_befp_validate_device(cda_ctx* ctx, uint32_t k, uint32_t nproofs, const void* d_descs, const void* d_entries,
                             uint32_t nentries, const void* d_shares, const void* d_nodes, uint32_t nnodes_total,
                             const void* d_roots, uint32_t nroots, void* d_verdicts, void* stream);

/* ---- a square rebuilt from proved samples: place, repair, retain ---- */
/* What a reconstructing full node does between sampling and serving (rsmt2d has no assemble step: it is handed
 * a square with holes; the rule below is this library's, the Repair and the commitment under it are rsmt2d's
 * (*ExtendedDataSquare).Repair and da.NewDataAvailabilityHeader as cda_repair and cda_square_open_eds run them).
 * Sample p: the cell (index, pos) proved in row tree `index` (axis CDA_AXIS_ROW), or the cell (pos, index) proved in
 * column tree `index` (CDA_AXIS_COL); its share is shares[512 p, 512 p + 512), its proof of leaf [pos, pos + 1) the
 * nodes[node_off, node_off + nnodes) of 90 B.  The namespace its leaf hashes under is derived: the share's first 29
 * bytes if index < k and pos < k, else 0xFF x 29. */
typedef struct {
  uint32_t axis, index, pos, node_off, nnodes;
} cda_sample_desc;
/* statuses[p], one byte per sample.  The lowest-indexed verified sample of a cell is placed, so the result does not
 * depend on the order of execution. */
#define CDA_SAMPLE_PLACED 0    /* verified, the lowest-indexed verified sample of its cell: its bytes are the cell */
#define CDA_SAMPLE_DUPLICATE 1 /* verified, not the lowest, the same bytes as the placed sample */
#define CDA_SAMPLE_CONFLICT 2  /* verified, not the lowest, other bytes: the cell is committed differently in its row
                                  tree and its column tree; the placed bytes stay the lowest-indexed sample's */
#define CDA_SAMPLE_REJECTED 3  /* nmt Proof.VerifyInclusion is false (nodes outside the total included) */
#define CDA_SAMPLE_MALFORMED 4 /* axis > 1, index >= 2k or pos >= 2k: nothing is read through it */
/* Verify and place only, every pointer device memory, asynchronous on `stream`: d_eds ((2k)^2 x 512 B) receives the
 * placed cells and zeros elsewhere, d_present ((2k)^2 bytes) 1 for a placed cell, d_statuses (nsamples bytes) the
 * CDA_SAMPLE_* of every sample.  d_roots: 4k x 90 B, the row roots then the column roots.  d_shares and d_eds must be
 * 16-byte aligned, the others 4-byte aligned, else CDA_E_ARG; k a power of two (CDA_E_NOT_POW2), k <= 512
 * (CDA_E_UNSUPPORTED).  nsamples == 0 is legal: nothing is present.  Uses the context's workspace. */
int cda_samples_assemble_device(cda_ctx* ctx, uint32_t k, uint32_t nsamples, const void* d_descs, const void* d_shares,
                                const void* d_nodes, uint32_t nnodes_total, const void* d_roots, void* d_eds,
                                void* d_present, void* d_statuses, void* stream);
/* cda_square_open_eds for a square already in this GPU's memory (the output of cda_repair_device or
 * cda_extend_commit_device; 16-byte aligned): one device-to-device copy into the handle, ordered after prior work on
 * `stream`, then the same commitment with the same outputs; returns when the handle is complete. */
int cda_square_open_eds_device(cda_ctx* ctx, uint32_t k, const void* d_eds, cda_square** out, uint8_t* row_roots,
                               uint8_t* col_roots, uint8_t* dah, cda_err_info* err, void* stream);
/* The whole chain from host buffers: the samples are staged and assembled straight into a new handle's memory,
 * repaired there against the given roots (rsmt2d Repair, as cda_repair) and committed in place; the square itself
 * never crosses the bus unless eds_or_null asks for it.
 *   CDA_OK              *out is the handle, dah its data root; the handle's roots equal row_roots / col_roots.
 *   CDA_E_UNREPAIRABLE, CDA_E_BYZANTINE (err->axis / index)
 *                       *out is NULL; present_or_null and eds_or_null receive the state where rsmt2d stops, as
 *                       cda_repair returns it.
 * statuses (nsamples bytes) is written whenever the samples were assembled; present_or_null ((2k)^2 bytes) and
 * eds_or_null ((2k)^2 x 512 B) are optional.  CDA_E_ARG, CDA_E_NOT_POW2 and CDA_E_UNSUPPORTED (k > 512) come before
 * any device work. */
int cda_square_rebuild(cda_ctx* ctx, uint32_t k, uint32_t nsamples, const cda_sample_desc* descs,
                       const uint8_t* shares, const uint8_t* nodes, uint32_t nnodes_total, const uint8_t* row_roots,
                       const uint8_t* col_roots, cda_square** out, uint8_t* statuses, uint8_t* present_or_null,
                       uint8_t* eds_or_null, uint8_t* dah, cda_err_info* err);

/* ---- halves of rows and columns: serve, verify, rebuild (celestia-node shwap.Row / Row.Verify) ---- */
/* Half p: the k consecutive cells [side k, side k + k) of row `index` (axis CDA_AXIS_ROW) or of column `index`
 * (CDA_AXIS_COL) of a 2k x 2k square, sent with no proof; its shares are shares[512 k p, 512 k (p + 1)) in cell
 * order; the roots of its block are roots[root_off, root_off + 4k) of 90 B, the 2k row roots then the 2k column
 * roots (cda_befp_desc's layout).  The receiver completes the axis with the codec (side 0: cells [k, 2k) are the
 * encoding of cells [0, k); side 1: cells [0, k) are decoded from exactly the cells [k, 2k)), builds the wrapper
 * tree (squareSize k, axisIndex index; a cell's namespace is its own first 29 bytes if index < k and its position
 * < k, else 0xFF x 29) over the 2k cells and compares its root with the committed one.  Row.Verify lives in
 * celestia-node, outside the pinned tree: this is the library's statement of it. */
#define CDA_SIDE_FIRST 0  /* cells [0, k) of the axis */
#define CDA_SIDE_SECOND 1 /* cells [k, 2k) */
typedef struct {
  uint32_t axis, index, side, root_off;
} cda_axis_half_desc;
/* statuses[p], one byte per half, the first check that applies deciding; a false half is a status, never an error
 * code.  DUPLICATE and CONFLICT occur only where a square is assembled. */
#define CDA_HALF_PLACED 0    /* verified (what cda_axis_halves_verify returns for a half that verifies); assembling:
                                the lowest-indexed verified half of its axis, its bytes are every cell it owns */
#define CDA_HALF_DUPLICATE 1 /* verified, a lower-indexed verified half has the same axis (either side of it) */
#define CDA_HALF_CONFLICT 2  /* verified and its axis's half, but at a cell owned by a lower-indexed half its bytes
                                differ: a row tree and a column tree commit one cell differently; it still places
                                the cells it owns */
#define CDA_HALF_BAD_ROOT 3  /* the tree cannot be built (push order) or its root is not the committed one */
#define CDA_HALF_MALFORMED 4 /* axis > 1, index >= 2k, side > 1 or root_off + 4k > nroots (assembling: root_off != 0):
                                nothing is read through it */
/* Serve: nq halves out of a retained square, packed in query order, k x 512 B each (root_off is ignored).  `shares`
 * may be host or device memory, as cda_square_prove's outputs; shares_cap in bytes.  CDA_E_ARG if it is too small or
 * a query lies outside the square, before anything is launched. */
int cda_square_axis_halves(cda_square* sq, uint32_t nq, const cda_axis_half_desc* q, uint8_t* shares,
                           uint64_t shares_cap);
/* Batched Row.Verify: statuses[p] is CDA_HALF_PLACED (= verified), CDA_HALF_BAD_ROOT or CDA_HALF_MALFORMED.
 * axes_or_null receives the completed axes, nhalves x 2k x 512 B (the bytes of an axis that is not verified are
 * unspecified, but written inside its slot).  All halves of a call share k (a power of two, else CDA_E_NOT_POW2;
 * k <= 512 and nhalves x 2k < 2^31, else CDA_E_UNSUPPORTED); they may belong to different blocks through root_off.
 * nhalves == 0 is legal. */
int cda_axis_halves_verify(cda_ctx* ctx, uint32_t k, uint32_t nhalves, const cda_axis_half_desc* descs,
                           const uint8_t* shares, const uint8_t* roots, uint32_t nroots, uint8_t* statuses,
                           uint8_t* axes_or_null);
/* The same with every pointer in device memory (d_shares and d_axes_or_null 16-byte, the others 4-byte aligned, else
 * CDA_E_ARG), asynchronous on `stream`; every check is made in the kernels.  Uses the context's workspace. */
int cda_axis_halves_verify_device(cda_ctx* ctx, uint32_t k, uint32_t nhalves, const void* d_descs,
                                  const void* d_shares, const void* d_roots, uint32_t nroots, void* d_statuses,
                                  void* d_axes_or_null, void* stream);
/* Verify and place, every pointer device memory, asynchronous on `stream`, as cda_samples_assemble_device: all halves
 * belong to the one square whose roots are d_roots (4k x 90 B; root_off must be 0); d_eds ((2k)^2 x 512 B) and
 * d_present ((2k)^2 bytes) are cleared first and receive every cell of every placed axis -- all 2k cells of the
 * completed axis, not only the k that were sent; d_statuses (nhalves bytes) the CDA_HALF_* of every half.  d_shares
 * and d_eds 16-byte, the others 4-byte aligned, else CDA_E_ARG.  nhalves == 0 is legal: nothing is present. */
int cda_axis_halves_assemble_device(cda_ctx* ctx, uint32_t k, uint32_t nhalves, const void* d_descs,
                                    const void* d_shares, const void* d_roots, void* d_eds, void* d_present,
                                    void* d_statuses, void* stream);
/* The whole chain from host buffers, as cda_square_rebuild: the halves are staged and assembled straight into a new
 * handle's memory, repaired there against the given roots (rsmt2d Repair) and committed in place.  Return codes and
 * the meaning of out / statuses / present_or_null / eds_or_null / dah / err are cda_square_rebuild's. */
int cda_square_rebuild_axes(cda_ctx* ctx, uint32_t k, uint32_t nhalves, const cda_axis_half_desc* descs,
                            const uint8_t* shares, const uint8_t* row_roots, const uint8_t* col_roots,
                            cda_square** out, uint8_t* statuses, uint8_t* present_or_null, uint8_t* eds_or_null,
                            uint8_t* dah, cda_err_info* err);

/* ---- square construction on the device (go-square square.Construct + shares.ToBytes) ---- */
/* The step before the DA path (app/prepare_proposal.go:54,65, app/process_proposal.go:121,137): the
 * host plans the layout -- which sequence or blob goes where, the PFB share indexes, the compact
 * reserved offsets -- as share segments; libcda writes the k*k shares straight into device memory
 * (specs/src/specs/shares.md) and, in cda_construct_extend_commit, extends and commits them.  Segments
 * are sorted by first_share and tile [0, k*k) exactly. */
enum { CDA_SEG_COMPACT = 0, CDA_SEG_SPARSE = 1, CDA_SEG_PADDING = 2 };
typedef struct {
  uint32_t kind;          /* CDA_SEG_* */
  uint32_t first_share;   /* row-major ODS index of the segment's first share */
  uint32_t nshares;
  uint32_t share_version; /* info byte = share_version << 1 | sequence start */
  uint64_t data_off;      /* COMPACT: varint-delimited sequence, SPARSE: blob data, in `data` */
  uint64_t data_len;      /* sequence length written in the first share (0 for padding) */
  uint32_t reserved_off;  /* COMPACT: index in `reserved` of the segment's first share */
  uint8_t ns[29];         /* namespace (version byte ‖ 28-byte ID) */
  uint8_t pad_[3];
} cda_share_segment;
/* Builds the ODS (k*k*512 bytes) of the plan into device memory d_ods on `stream` (asynchronous). */
int cda_build_ods_device(cda_ctx* ctx, uint32_t k, uint32_t nseg, const cda_share_segment* segs, const uint8_t* data,
                         uint64_t data_len, const uint32_t* reserved, uint32_t nreserved, void* d_ods, void* stream);
/* square.Construct + shares.ToBytes + da.ExtendShares + NewDataAvailabilityHeader in one call from a
 * host plan: only the payload bytes (sequences and blobs) cross PCIe.  Outputs as cda_extend_commit
 * (ods_or_null additionally receives the k*k shares). */
int cda_construct_extend_commit(cda_ctx* ctx, uint32_t k, uint32_t nseg, const cda_share_segment* segs,
                                const uint8_t* data, uint64_t data_len, const uint32_t* reserved, uint32_t nreserved,
                                uint8_t* ods_or_null, uint8_t* eds_or_null, uint8_t* row_roots, uint8_t* col_roots,
                                uint8_t* dah, cda_err_info* err);

/* ---- instrumentation ----------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by HIP events on its own
 * stream and per-kernel total time / launch counts are accumulated. */
int cda_profile_enable(cda_ctx* ctx, int enable);
/* Copies up to `cap` entries: names (NUL-separated into names_buf), total ms, launches. */
int cda_profile_read(cda_ctx* ctx, char* names_buf, size_t names_cap, double* total_ms, int64_t* launches,
                     int cap);
int cda_profile_reset(cda_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif
