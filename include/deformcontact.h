/*
 * deformcontact.h -- C ABI of libdeformcontact_hip.so (MI355X / gfx950).
 *
 * The drop-in boundary of the DeformContact message-passing hot path.  The
 * reference has no FFI of its own: its boundary is the PyG operator surface
 * called from /root/reference/models/model.py:45,49,71,77
 * (`conv_layer(in, out)`, `conv(x, edge_index)`), whose arithmetic is PyG 2.5.2's
 * gcn_norm + MessagePassing.propagate + Linear.  Each entry point below names
 * the PyG/ATen step it replaces.  The Python host (deformcontact_amd/) binds
 * these with ctypes, deriving every signature and DC_* limit from the
 * prototypes and #defines of this file ("Binding").
 *
 * Conventions
 *   - a pointer parameter is a DEVICE pointer owned by the caller (PyTorch)
 *     unless it is marked DC_HOST (a host array the call reads, or writes,
 *     before it returns), is a pointer to pointers (always a host array of
 *     device pointers) or is a `char *` (host text); the library allocates
 *     nothing and keeps no mutable global state except the thread-local
 *     last-error string;
 *   - every call only ENQUEUES work on `stream` (a hipStream_t); no call
 *     synchronises, so all of them are legal inside hipGraph capture;
 *   - return value 0 = enqueued, <0 = DC_E* (nothing enqueued), message in
 *     dc_last_error();
 *   - matrices are row-major fp32 with an explicit leading dimension (in
 *     elements); index arrays produced by the library are int32; the only int64
 *     input is PyG's `edge_index` [2,E].
 */
#ifndef DEFORMCONTACT_H
#define DEFORMCONTACT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DC_OK 0
#define DC_EINVAL (-1)   /* bad argument (null pointer, negative size, alignment) */
#define DC_ELAUNCH (-2)  /* hipLaunch / runtime error, text in dc_last_error()   */
#define DC_EWORKSPACE (-3)

typedef void *dc_stream_t; /* hipStream_t */
#define DC_HOST            /* marks a single-star pointer parameter that points to HOST memory (see Conventions) */

#define DC_MAX_PARTS 4     /* edge_index parts of one merged (block-diagonal) adjacency */
#define DC_MAX_GROUPS 4    /* row groups with their own weights in one grouped dense launch */
#define DC_GROUP_ALIGN 256 /* every group of a grouped launch starts at a multiple of this many rows */

int dc_version(void);
const char *dc_last_error(void);
/* Sequence id of the hipGraph capture `stream` currently takes part in, 0 when it is not
 * capturing.  The host's adjacency cache uses it: a sorted adjacency is only reused by the
 * capture that enqueued its build (the build has not RUN while a capture is open). */
int64_t dc_stream_capture_id(dc_stream_t stream);

/* ---- topology: edge_index -> sorted adjacency ("CSR") ---------------------
 * Replaces the implicit ordering of PyG's scatter_add_ (utils/_scatter.py) and,
 * with `w != NULL`, gcn_norm (nn/conv/gcn_conv.py) which the reference
 * recomputes in every conv call (model.py:71,77 -> TAGConv.forward).
 *
 * Groups the E edges by edge_index[key_row] (key_row = 1: by destination, the
 * forward CSR; key_row = 0: by source, the transposed set used by backward),
 * STABLY: inside a group edges keep their input order, i.e. the result equals
 * np.argsort(edge_index[key_row], kind="stable").  Bit-exact, deterministic.
 *
 *   self_loops = 0 : edge set used as is (TAGConv: gcn_norm(add_self_loops=False))
 *   self_loops = 1 : existing self loops dropped, one loop per node appended
 *                    with edge ids E..E+N-1 (GCNConv add_remaining_self_loops,
 *                    GATConv remove_self_loops + add_self_loops; utils/loop.py).
 *                    Output arrays must then hold E+N entries; the actual edge
 *                    count is ptr[N].
 *
 *   ptr   [N+1]  group offsets
 *   other [E']   the other endpoint of each sorted edge (source for key_row=1)
 *   perm  [E']   original edge id of each sorted edge
 *   w     [E']   optional: deg^-1/2[src] * deg^-1/2[dst], deg = in-degree
 *                counting duplicates, 0 for deg = 0.  `deg_ptr` = offsets whose
 *                differences give that in-degree: NULL = this call's own `ptr`
 *                (valid for key_row = 1), else the key_row=1 ptr of the same
 *                edge set.
 *   status[1]    device int32, SET by the call: 1 if any endpoint is outside [0,N)
 *                (such edges are skipped), else 0.  Read it back after synchronising.
 *   workspace    dc_csr_workspace_bytes(E, N) bytes, 16-byte aligned.
 *
 * Groups of any length are handled in O(S log^2 S) (hubs are sorted by one workgroup, short
 * groups ranked by counting): no quadratic walk on high-degree nodes.
 */
int64_t dc_csr_workspace_bytes(int64_t E, int64_t N);
int dc_csr_build(const int64_t *edge_index, int64_t E, int64_t N, int key_row,
                 int self_loops, int32_t *ptr, int32_t *other, int32_t *perm,
                 const int32_t *deg_ptr, float *w, int32_t *status, void *workspace,
                 int64_t workspace_bytes, dc_stream_t stream);

/* Both sides of one edge set in ONE pipeline (5 launches for N <= 65,536, 7 beyond): the
 * key_row = 1 set (`*_f`: by destination, the forward hop) and the key_row = 0 set (`*_b`: by
 * source, the transposed hop of the backward pass), identical to two dc_csr_build calls with
 * deg_ptr = ptr_f for the second.  w_f / w_b both NULL or both set.  This is what one
 * `conv(x, edge_index)` of the reference needs per NEW edge_index (model.py:71,77); it is cheap
 * enough (tens of microseconds at the batch-32 shape) to sit inside a captured training step.
 * Edge lists of 2^19 slots and more (E, + N with self loops) take the bucketed build - partition by
 * node bucket, one workgroup per bucket, no atomic per edge: the same arrays whatever the order of
 * the edges (a relabelled radius graph; env DC_CSR_BUCKETS = 0 / 1 forces the choice). */
int64_t dc_graph_workspace_bytes(int64_t E, int64_t N);
int dc_graph_build(const int64_t *edge_index, int64_t E, int64_t N, int self_loops,
                   int32_t *ptr_f, int32_t *other_f, int32_t *perm_f, float *w_f,
                   int32_t *ptr_b, int32_t *other_b, int32_t *perm_b, float *w_b,
                   int32_t *status, void *workspace, int64_t workspace_bytes, dc_stream_t stream);

/* dc_graph_build over a MERGED edge set: `nparts` (<= DC_MAX_PARTS) edge_index arrays
 * (edge_index_parts[p] = int64 [2, E_parts[p]]) read as one concatenated edge list - edge ids run
 * through the parts in order - over ONE node space of N nodes in which part p's node ids are
 * shifted by node_offset_parts[p] (ascending; part p must stay inside
 * [node_offset_parts[p], node_offset_parts[p] + nodes_parts[p]), which is also the range its ids
 * are checked against).  This is the block-diagonal union PyG's Batch.from_data_list builds per
 * graph type, taken one step further: the soft and the rigid graph of a batch (train.py:36-38)
 * in one adjacency, so that the conv layers of both encoder branches (models/model.py:69-78) run
 * as single launches.  Nodes that belong to no part (padding between parts) are isolated.  Rows
 * of part p come out exactly as dc_graph_build over that part alone would emit them (same stable
 * order, same gcn_norm weights), with `other` shifted by the part's offset and `perm` by the
 * part's first edge id. */
int dc_graph_build_parts(const int64_t *const *edge_index_parts, DC_HOST const int64_t *E_parts,
                         DC_HOST const int64_t *node_offset_parts, DC_HOST const int64_t *nodes_parts, int nparts,
                         int64_t N, int self_loops,
                         int32_t *ptr_f, int32_t *other_f, int32_t *perm_f, float *w_f,
                         int32_t *ptr_b, int32_t *other_b, int32_t *perm_b, float *w_b,
                         int32_t *status, void *workspace, int64_t workspace_bytes, dc_stream_t stream);

/* Which pipeline dc_csr_build / dc_graph_build / dc_graph_build_parts take for an edge set of this size (host only,
 * no HIP call): returns 1 = bucketed build, with *bucket_shift = log2 of the nodes per bucket and *buckets = buckets
 * per side; 0 = windowed pipeline (outputs untouched); DC_EINVAL for negative sizes.  The rule: at least
 * DC_CSR_BUCKETS_MIN slots (env, default 2^19; slots = E, + N with self loops), buckets such that an average
 * bucket fills at most a quarter of one 12,288-slot LDS pass, at most 2,048 nodes per bucket and 8,192 buckets.
 * (Diagnostic / test hook: nothing in the reference corresponds to it.) */
int dc_graph_build_plan(int64_t E, int64_t N, int self_loops, DC_HOST int *bucket_shift, DC_HOST int *buckets);

/* dc_graph_build for a BATCH of graphs whose layout is known (Batch.from_data_list, the loaders of
 * /root/reference/loaders/everyday.py:96 via torch_geometric.data.Batch): graph i owns nodes
 * [node_ptr[i], node_ptr[i+1]) and input edges [edge_ptr[i], edge_ptr[i+1]) and no edge leaves its
 * graph.  node_ptr / edge_ptr are HOST arrays of nseg + 1 int64 (ascending, from 0 to N / E; checked
 * here: DC_EINVAL otherwise, and when a graph exceeds DC_SEG_MAX_NODES / DC_SEG_MAX_EDGES); they
 * travel in the kernel arguments, so under hipGraph capture they are part of the captured launch.
 * One launch per 96 graphs - workgroup (graph, side) sorts the graph's edges in LDS - no workspace,
 * no global atomics; writes exactly the arrays dc_graph_build (self_loops = 0) writes, bit for bit.
 * status is only OR-ed into (the caller zeroes it once): bit 0 = an edge leaves its graph (the arrays
 * then hold in-range but meaningless entries, as with an out-of-range id); a flag survives rebuilds
 * until the caller clears it. */
#define DC_SEG_MAX_NODES 4096
#define DC_SEG_MAX_EDGES 16384
int dc_graph_build_segmented(const int64_t *edge_index, int64_t E, int64_t N,
                             DC_HOST const int64_t *node_ptr_host, DC_HOST const int64_t *edge_ptr_host, int nseg,
                             int32_t *ptr_f, int32_t *other_f, int32_t *perm_f, float *w_f,
                             int32_t *ptr_b, int32_t *other_b, int32_t *perm_b, float *w_b,
                             int32_t *status, dc_stream_t stream);
/* dc_graph_build_segmented that also writes, per side, the table image dc_hop_chain_image_f32 reads instead of
 * deriving its LDS tables from ptr / other / deg_ptr in every workgroup: the same launch, no more LDS, no atomics.
 * An image holds dc_hop_chain_image_bytes(N) bytes (16-byte aligned):
 *     ids    [N][8] uint16   the first eight neighbours of every row as ids local to its graph, in `other` order;
 *                            slots behind the row's last neighbour hold 0xffff
 *     bounds [N][2] int32    {ptr[row], ptr[row + 1] - ptr[row]}
 *     dis    [N + 1] float   in-degree^-1/2 (0 for degree 0) of every node; entry N, which a pad id stands for, is 0
 * each table at its offset in that order.  Values are those the chain kernel computes itself, bit for bit (an edge the
 * build flags sits on its graph's node 0 in the image as in `other`). */
int64_t dc_hop_chain_image_bytes(int64_t N);
int dc_graph_build_segmented_image(const int64_t *edge_index, int64_t E, int64_t N,
                                   DC_HOST const int64_t *node_ptr_host, DC_HOST const int64_t *edge_ptr_host, int nseg,
                                   int32_t *ptr_f, int32_t *other_f, int32_t *perm_f, float *w_f,
                                   int32_t *ptr_b, int32_t *other_b, int32_t *perm_b, float *w_b,
                                   void *image_f, void *image_b, int32_t *status, dc_stream_t stream);
/* The self_loops = 1 form (the host layer takes it for small batches of GATConv(edge_dim) only), same arguments and caps; output arrays hold E + N entries.
 * Input self loops are dropped and the loop of node i is appended with edge id E + i, last in its group; the edge count
 * is ptr[N].  Still one launch per 96 graphs and no workspace: every workgroup counts the self loops among the input
 * edges in front of its graph itself.  Writes the arrays dc_graph_build (self_loops = 1) writes up to ptr[N], bit for
 * bit (gcn_norm degrees count the loop).  An edge that leaves its graph is flagged in status and kept as an edge of the
 * graph's first node; a self loop outside its graph's node range is flagged and dropped.  The count costs a read of
 * nseg * E / 2 edges per side: meant for small batches. */
int dc_graph_build_segmented_loops(const int64_t *edge_index, int64_t E, int64_t N,
                                   DC_HOST const int64_t *node_ptr_host, DC_HOST const int64_t *edge_ptr_host, int nseg,
                                   int32_t *ptr_f, int32_t *other_f, int32_t *perm_f, float *w_f,
                                   int32_t *ptr_b, int32_t *other_b, int32_t *perm_b, float *w_b,
                                   int32_t *status, dc_stream_t stream);

/* 30-bit Morton (Z-order) code of every point of pos [n, >=3] (fp32, leading dimension ld): each
 * axis is mapped from [lo[a], lo[a] + 1 / inv_extent[a]) to 10 bits (lo / inv_extent are HOST
 * arrays of 3 floats).  The host sorts nodes by it (graph.NodeOrder.morton) so that the rows a
 * radius-graph hop gathers (utils/pointcloud_utils.py:10) are neighbours in memory. */
int dc_morton_codes(const float *pos, int64_t ld, int64_t n, DC_HOST const float *lo_host,
                    DC_HOST const float *inv_extent_host, int64_t *codes, dc_stream_t stream);

/* ---- node reordering of one big graph, on the device (dc_order.hip; BASELINE.json configs[4]) ----
 * dc_morton_order: Z-order permutation of a point cloud pos [n, >= 3] (fp32, leading dimension ld): the bounding
 *   box, the 30-bit codes (10 bits per axis over its extent), a STABLE key sort (rocPRIM device radix sort) and the
 *   inverse - perm[new] = old, inv[old] = new (int32) - without a host synchronisation (hipGraph-capturable).
 *   Running a conv stack on gather_rows(x, perm) / relabel(edge_index) and putting the result back with
 *   gather_rows(y, inv) turns the hops' neighbour gathers of a radius graph (utils/pointcloud_utils.py:10) into reads
 *   of nearby rows; outputs are bit-identical to the unordered run (a row's neighbours stay in edge order).
 * dc_relabel_edges: out[i] = inv[ei[i]] over `count` int64 ids (both rows of edge_index at once).
 * dc_gather_rows  : out row i = x row idx[i], rows of row_bytes bytes (a multiple of 16; any element type). */
int64_t dc_morton_order_workspace_bytes(int64_t n);
int dc_morton_order(const float *pos, int64_t ld, int64_t n, int32_t *perm, int32_t *inv, void *workspace,
                    int64_t workspace_bytes, dc_stream_t stream);
int dc_relabel_edges(const int64_t *ei, int64_t count, const int32_t *inv, int64_t n, int64_t *out,
                     dc_stream_t stream);
int dc_gather_rows(const void *x, int64_t ldx_bytes, const int32_t *idx, void *out, int64_t ldo_bytes, int64_t n,
                   int64_t row_bytes, dc_stream_t stream);

/* ---- kNN / radius neighbour search (dc_neighbors.hip; PyG knn, knn_graph, radius, radius_graph) ----
 * dc_neighbors_fill: for every query point y[i] (fp32 [ny, >= 3], leading dimension ldy) its neighbours among the
 *   points x[j] (fp32 [nx, >= 3], ldx) of the same graph:
 *     batch_x [nx], batch_y [ny]: sorted int64 graph ids, or NULL for "all in graph 0";
 *     d2 = ((dx*dx + dy*dy) + dz*dz), dx = x_j - y_i, every product and sum rounded on its own in fp32;
 *     the candidates are ranked by (d2, j) ascending; mode DC_NEIGHBORS_KNN keeps the first `cap`,
 *     DC_NEIGHBORS_RADIUS the first `cap` of those with d2 < r*r (r*r rounded once in fp32);
 *     exclude_self != 0 drops j == i (by index: a duplicate point j != i stays, at distance 0).
 *   Writes counts[i] (int32) and nbr [ny, cap] (int32, row i = the neighbours in rank order, then -1).
 *   0 <= cap <= DC_NEIGHBORS_MAX_CAP.  The result depends on no atomic order: two calls are bit-identical.
 *   Workspace: dc_neighbors_workspace_bytes(nx, ny) bytes, 16-byte aligned (0 when nx = 0).
 * dc_neighbors_compact: the exact edge list of such a fill: an inclusive scan of the counts (rocPRIM) and the
 *   scatter of row i's counts[i] neighbours to edges [offset(i), offset(i) + counts[i]) of
 *   edge_index [2, num_edges] (int64, row length num_edges): row `query_row` gets i, the other row the neighbour.
 *   num_edges is the counts' total, which the caller reads; edges beyond it are not written.
 *   Workspace: dc_neighbors_compact_workspace_bytes(ny) bytes. */
#define DC_NEIGHBORS_MAX_CAP 64
#define DC_NEIGHBORS_KNN 0
#define DC_NEIGHBORS_RADIUS 1
int64_t dc_neighbors_workspace_bytes(int64_t nx, int64_t ny);
int dc_neighbors_fill(const float *x, int64_t ldx, int64_t nx, const int64_t *batch_x, const float *y, int64_t ldy,
                      int64_t ny, const int64_t *batch_y, int mode, float r, int cap, int exclude_self, int32_t *nbr,
                      int32_t *counts, void *workspace, int64_t workspace_bytes, dc_stream_t stream);
int64_t dc_neighbors_compact_workspace_bytes(int64_t ny);
int dc_neighbors_compact(const int32_t *nbr, int cap, const int32_t *counts, int64_t ny, int query_row,
                         int64_t *edge_index, int64_t num_edges, void *workspace, int64_t workspace_bytes,
                         dc_stream_t stream);

/* ---- kNN over rows of any width (dc_neighbors_nd.hip; PyG knn / knn_graph in feature space, DynamicEdgeConv) ----
 * dc_neighbors_nd_fill: dc_neighbors_fill's kNN mode for x fp32 [nx, f] and y fp32 [ny, f], f >= 1 (unit inner
 *   stride, leading dimensions ldx, ldy >= f): an exact tiled brute force per graph, no grid and no workspace.
 *     batch_x [nx], batch_y [ny]: sorted int64 graph ids, or NULL for "all in graph 0"; a query's candidates are
 *       the rows of x with its own graph id, found on the device;
 *     with d_c = x[j,c] - y[i,c]: d2 = d_0*d_0, then d2 = d2 + d_c*d_c for c = 1 .. f-1 IN COLUMN ORDER, every
 *       difference, product and sum rounded on its own in fp32 (f = 3: the rule of dc_neighbors_fill, bit for bit);
 *       never the |x|^2 + |y|^2 - 2 x.y form, never MFMA;
 *     the candidates are ranked by (d2, j) ascending and the first `cap` kept; exclude_self != 0 drops j == i by
 *       index (a duplicate row j != i stays, at distance 0).
 *   Writes counts [ny] and nbr [ny, cap] in exactly dc_neighbors_fill's layout (rank order, then -1), so
 *   dc_neighbors_compact and every other consumer take them unchanged.  0 <= cap <= DC_NEIGHBORS_MAX_CAP.  No atomics:
 *   two calls are bit-identical.  Non-finite features: the ranking is unspecified; the kernel terminates and stays in
 *   bounds.  Errors (DC_EINVAL before any HIP call): bad sizes, f < 1, ld < f, a null pointer with work to do.
 *   ny == 0 returns DC_OK at once; cap == 0 writes the zero counts where counts is given and returns DC_OK; with
 *   nx == 0 every count is 0.
 *   DC_NEIGHBORS_ND_CHUNK: the columns the kernel stages per pass over a candidate tile (widths below, at and above
 *   it and its multiples take different code paths: the tests read it). */
#define DC_NEIGHBORS_ND_CHUNK 32
int dc_neighbors_nd_fill(const float *x, int64_t ldx, int64_t nx, const int64_t *batch_x, const float *y, int64_t ldy,
                         int64_t ny, const int64_t *batch_y, int64_t f, int cap, int exclude_self, int32_t *nbr,
                         int32_t *counts, dc_stream_t stream);

/* Order-dependent 64-bit content hash of an int64 device array (e.g. edge_index) into
 * out[1] (device): the key of the host's per-topology cache (loaders.TopologyCache), so a batch
 * whose edge_index has been seen before reuses its sorted adjacency. */
int dc_hash_i64(const int64_t *v, int64_t n, uint64_t *out, dc_stream_t stream);

/* ---- the hop: fused gather - scale - segment-sum --------------------------
 * Replaces MessagePassing.propagate for aggr="add" with message = w_e * x_j:
 * index_select(x, 0, row) -> mul -> zeros(N,F).scatter_add_(0, col) (three ATen
 * ops and two [E,F] temporaries per hop in PyG).
 *
 *   y[i, 0:F] = (addend ? addend[i, 0:F] : 0)
 *             + sum over p in [ptr[i], ptr[i+1]) of  w[p] * x[other[p], 0:F]
 *
 * summed in p order with separately rounded multiply and add, so the result is
 * bit-identical to a serial walk over the stably sorted edges.  w == NULL means
 * weight 1.  Forward passes the key_row=1 set, backward the key_row=0 set
 * (y = A_hat^T g + addend).  y must not alias x; y may alias addend.
 */
int dc_spmm_f32(const int32_t *ptr, const int32_t *other, const float *w, const float *x,
                int64_t ldx, const float *addend, int64_t ldadd, float *y, int64_t ldy,
                int64_t N, int64_t F, dc_stream_t stream);

/* dc_tag_pack_input + the FIRST hop of a narrow layer's own input in one launch (F <= 32: the encoder's first TAGConv,
 * models/model.py:71,77 with the raw graph.x): slab[i, 0:F] = x[i, 0:F], slab[i, F:2F] = sum_p w[p] x[other[p], 0:F]
 * (terms and order of dc_spmm_f32), slab[i, width:wpad] = 0.  One launch less on the chain of small dependent kernels
 * a new batch starts with. */
int dc_spmm_f32_pack(const int32_t *ptr, const int32_t *other, const float *w, const float *x, int64_t ldx,
                     float *slab, int64_t lds, int64_t N, int64_t F, int64_t width, int64_t wpad,
                     dc_stream_t stream);
/* ... and, in the same launch, the weight image of the layer's forward block (dc_tag_narrow_wimage below: ws, nseg with
 * nseg * F = width, wimg; wpad = 96 / 112 / 128): a few more workgroups prepare it once per call. */
int dc_spmm_f32_pack_wprep(const int32_t *ptr, const int32_t *other, const float *w, const float *x, int64_t ldx,
                           float *slab, int64_t lds, int64_t N, int64_t F, int64_t width, int64_t wpad,
                           const float *const *ws, int nseg, void *wimg, dc_stream_t stream);

/* dc_spmm_f32 over a ROW WINDOW of a merged adjacency (dc_graph_build_parts): `ptr` points at the
 * window's first row (N + 1 entries; its values index the full other / w arrays), neighbour ids are
 * ids of the merged node space, and x / addend / y hold only the window's N rows: the neighbour
 * row read is other[p] - row_offset.  Lets one part of a merged graph (e.g. the first, narrow
 * layer of one encoder branch) hop over its own feature matrix without a second adjacency. */
int dc_spmm_f32_window(const int32_t *ptr, const int32_t *other, const float *w, const float *x,
                       int64_t ldx, const float *addend, int64_t ldadd, float *y, int64_t ldy,
                       int64_t N, int64_t F, int64_t row_offset, dc_stream_t stream);
/* ... and with the row maxima of dc_spmm_f32_rowmax (rowmax holds the window's N rows). */
int dc_spmm_f32_rowmax_window(const int32_t *ptr, const int32_t *other, const float *w, const float *x,
                              int64_t ldx, const float *addend, int64_t ldadd, float *y, int64_t ldy,
                              int64_t N, int64_t F, float *rowmax, int mode, int64_t row_offset,
                              dc_stream_t stream);

/* The same hop over bf16-STORED feature rows ("bf16 features, fp32
 * accumulate"; PyG reaches it as conv(x.bfloat16(), edge_index) under autocast, where
 * index_select/mul/scatter_add_ run in bf16 -- this entry keeps the sum in fp32 instead).
 * x is bf16 (uint16 bit patterns, row-major, ldx in elements).  Every term is
 * fp32(w[p]) * fp32(x[other[p]]) with the running sum in fp32, rounded and ordered exactly as
 * dc_spmm_f32.  y_is_f32 != 0: y / addend are fp32 and receive the fp32 sum; y_is_f32 == 0:
 * y / addend are bf16 and the sum is rounded ONCE, to nearest even, on store.  Half the gather
 * bytes of the fp32 hop: algorithmic bytes E*(8 + 2F) + N*(sizeof(y)*F + 4). */
int dc_spmm_bf16(const int32_t *ptr, const int32_t *other, const float *w, const uint16_t *x,
                 int64_t ldx, const void *addend, int64_t ldadd, void *y, int64_t ldy, int64_t N,
                 int64_t F, int y_is_f32, dc_stream_t stream);

/* dc_spmm_f32 that also records the row maxima the fp16x2 dense block scales by:
 * rowmax[i] = max |y[i,:]|, joined with max |x[i,:]| (the row's own input) when mode & 1 and with
 * the value rowmax[i] already holds when mode & 2.  y is bit-identical to dc_spmm_f32. */
int dc_spmm_f32_rowmax(const int32_t *ptr, const int32_t *other, const float *w, const float *x,
                       int64_t ldx, const float *addend, int64_t ldadd, float *y, int64_t ldy,
                       int64_t N, int64_t F, float *rowmax, int mode, dc_stream_t stream);

/* ---- K chained hops of a batch of small graphs in ONE launch (dc_hopchain.hip) ---------------
 * TAGConv.forward's K dependent propagate calls (PyG nn/conv/tag_conv.py, reached from
 * models/model.py:71,77) over a batch whose layout is known (Batch.from_data_list, train.py:36-38):
 * graph i owns the contiguous node range [node_ptr_host[i], node_ptr_host[i+1]) and none of its
 * edges leaves it (the layout dc_graph_build_segmented takes).  `slab` is the [N, ld] hop slab of a
 * layer, column block j = slab[:, j*F : (j+1)*F]; the call computes, for k = 1..K,
 *     block (src_block + k*dir)  =  A_hat . block (src_block + (k-1)*dir)
 * with every graph's 32-column slice resident in LDS for the whole chain - memory traffic: block
 * src_block in once, K blocks out once - and terms, order and rounding of dc_spmm_f32, so every
 * block is bit-identical to K dc_spmm_f32 calls.  rowmax != NULL: rowmax[i] = max over the K
 * produced blocks of max |block[i, :]|, joined with block src_block's when mode & 1 and with the
 * value rowmax[i] already holds when mode & 2 (what K dc_spmm_f32_rowmax calls leave there).
 * `cap` = number of elements `other` / `w` hold (16-byte id / weight loads are range-checked
 * against it).  deg_ptr != NULL (int32 [N+1]) states that the weights are gcn_norm's without self
 * loops, w[p] = d(source)^-1/2 * d(destination)^-1/2 with d(v) = deg_ptr[v+1] - deg_ptr[v] (the
 * in-degree: ptr of the by-destination set, for BOTH sets of dc_graph_build*): the kernel then
 * re-forms them from an LDS-resident table instead of loading them (same bits) and its hop loop
 * is free of vector-memory loads.  Needs F % 32 == 0, ld % 4 == 0, a 16-byte aligned slab and at most
 * dc_hop_chain_max_nodes() (4096: 32-column slices up to 1,024 nodes, 16-column ones up to 2,048, 8-column ones beyond; the
 * LDS-table form only with 32-column slices) nodes per graph; DC_EINVAL otherwise (use dc_spmm_f32). */
int64_t dc_hop_chain_max_nodes(void);
/* Bytes of LDS every dc_hop_chain_f32 workgroup requests: the WHOLE LDS of a compute unit (160 KiB), whatever its slice
 * needs, so that no LDS-using workgroup of another kernel can be resident beside it (round 5: with LDS left free, a
 * co-resident workgroup of a stock attention kernel on another stream made small chain workgroups return wrong elements
 * in 0.3 - 1.75 % of two-stream train steps; profiles/r05/README.md). */
int64_t dc_hop_chain_lds_request(void);
int dc_hop_chain_f32(const int32_t *ptr, const int32_t *other, const float *w, const int32_t *deg_ptr,
                     int64_t cap, DC_HOST const int64_t *node_ptr_host, int nseg, float *slab, int64_t ld, int64_t N,
                     int64_t F, int K, int src_block, int dir, float *rowmax, int mode,
                     dc_stream_t stream);
/* dc_hop_chain_f32 with the table image of the set it walks (image_f of dc_graph_build_segmented_image for the
 * by-destination set, image_b for the transposed one): with deg_ptr != NULL and 32-column slices every workgroup copies
 * its graph's tables from the image instead of building them from ptr / other / deg_ptr; same blocks and row maxima,
 * bit for bit.  image == NULL, or a launch that does not take the LDS-table form: exactly dc_hop_chain_f32. */
int dc_hop_chain_image_f32(const int32_t *ptr, const int32_t *other, const float *w, const int32_t *deg_ptr,
                           int64_t cap, DC_HOST const int64_t *node_ptr_host, int nseg, float *slab, int64_t ld, int64_t N,
                           int64_t F, int K, int src_block, int dir, float *rowmax, int mode, const void *image,
                           dc_stream_t stream);

/* ---- the dense block over bf16-STORED features (BASELINE.json configs[4]) ------------------
 * out[N,Fo] = act(A[N,K] . W[Fo,K]^T + bias) with A and W bf16 (uint16 bit patterns, K-contiguous,
 * K % 32 == 0, 16-byte aligned, lda % 8 == 0), fp32 accumulate on v_mfma_f32_32x32x16_bf16, out
 * fp32 (out_is_bf16 = 0) or bf16 rounded to nearest even (the next layer's hop slab).  A is the hop
 * slab dc_spmm_bf16 leaves, W the layer's lins[k].weight concatenated along K by dc_to_bf16.  This is
 * the precision PyG reaches under torch.autocast(bfloat16) (nn/dense/linear.py -> F.linear in bf16),
 * not the fp32-accurate split forms above. */
int dc_tag_linear_fwd_bf16(const uint16_t *a, int64_t lda, const uint16_t *w, const float *bias,
                           int relu, void *out, int64_t ldo, int out_is_bf16, int64_t N, int64_t K,
                           int64_t Fo, dc_stream_t stream);
/* Backward of that layer (configs[4] is fwd + bwd): the input gradient runs in the forward's shape -
 * dc_tag_mask_grad_bf16 writes gm = g * (out > 0) as bf16 into block 0 of a gradient slab (g / out_for_mask bf16 or
 * fp32 as flagged), K transposed dc_spmm_bf16 hops fill the other blocks, and dc_tag_linear_fwd_bf16 over that slab
 * with the transposed weights (dc_tag_transpose_weights + dc_to_bf16) gives gx.  dc_tag_linear_bwd_dw_bf16: the weight
 * gradients gws[s] [Fo, Fi] fp32 (the master weights stay fp32) = gm^T . x_s over the bf16 hop slab x [N, nseg * Fi]
 * (+ gbias [Fo] = column sums of gm), fp32 accumulate on v_mfma_f32_32x32x16_bf16, per node chunk with the partial
 * slabs summed in chunk order (deterministic); accumulate != 0 adds into gws / gbias.  Needs Fo % 128 == 0,
 * Fi % 256 == 0, 16-byte aligned rows; any N. */
int dc_tag_mask_grad_bf16(const void *g, int64_t ldg, int g_is_bf16, const void *out_for_mask, int64_t ldo,
                          int mask_is_bf16, uint16_t *gm, int64_t ldgm, int64_t N, int64_t F,
                          dc_stream_t stream);
int64_t dc_tag_linear_bwd_dw_bf16_workspace_bytes(int64_t N, int64_t Fi, int64_t Fo, int nseg);
int dc_tag_linear_bwd_dw_bf16(const uint16_t *g, int64_t ldg, const uint16_t *x, int64_t ldx, int nseg,
                              float *const *gws, float *gbias, int accumulate, void *partials,
                              int64_t partials_bytes, int64_t N, int64_t Fi, int64_t Fo, dc_stream_t stream);
/* dst[r, s*cols + c] = bf16(srcs[s][r, c]) (round to nearest even): fp32 matrices [rows, cols]
 * (leading dimension ld_src) concatenated along the columns into one bf16 matrix. */
int dc_to_bf16(const float *const *srcs, int nseg, int64_t rows, int64_t cols, int64_t ld_src,
               uint16_t *dst, int64_t ld_dst, dc_stream_t stream);

/* ---- the two training losses (train.py:51-53) ------------------------------------------------
 * losses[0] = L1Loss(pred, target) = mean |pred - target| over the [N,3] positions (train.py:51);
 * losses[1] = GradientConsistencyLoss (models/losses.py:7-19) = (1/E) sum over edges of
 *             || (target[dst] - target[src]) - (pred[dst] - pred[src]) ||_2 ;
 * grad_l1 / grad_gcl [N,3] = their gradients w.r.t. pred (zero gradient at a zero edge norm, as
 * torch's norm backward).  One pass over the nodes through BOTH sorted adjacencies of the edge set
 * (the *_f / *_b arrays of dc_graph_build; weights unused), deterministic two-stage sums, no float
 * atomics.  Replaces ~20 ATen launches (4 row gathers, norm, sums, L1 and their backward). */
int64_t dc_contact_loss_workspace_bytes(int64_t N);
int dc_contact_loss(const int32_t *ptr_f, const int32_t *other_f, const int32_t *ptr_b,
                    const int32_t *other_b, const float *pred, int64_t ld_pred, const float *target,
                    int64_t ld_target, int64_t N, int64_t E, float *grad_l1, float *grad_gcl,
                    float *losses /* [2] */, void *workspace, int64_t workspace_bytes,
                    dc_stream_t stream);

/* ---- dense block of TAGConv ------------------------------------------------
 * Replaces `out = lins[0](x); out = out + lins[k](x_k) ...; out = out + bias`
 * (nn/conv/tag_conv.py forward) = up to DC_MAX_SEG bias-free F.linear calls,
 * adds, and the optional ReLU of model.py:71,77, as ONE fp32-MFMA kernel:
 *
 *   out[N,Fo] = act( sum_s  xs[s][N,Fi] . ws[s][Fo,Fi]^T  + bias )
 *
 * xs[s] has leading dimension ldxs[s]; ws[s] is PyG's Linear.weight layout
 * [Fo,Fi] (ld = Fi).  Exact fp32 (v_mfma_f32_32x32x2_f32 is an fmaf chain).
 */
#define DC_MAX_SEG 4
int dc_tag_linear_fwd(const float *const *xs, DC_HOST const int64_t *ldxs, const float *const *ws,
                      int nseg, const float *bias, int relu, float *out, int64_t ldo,
                      int64_t N, int64_t Fi, int64_t Fo, dc_stream_t stream);

/* dX-side of the backward:  gxs[s][N,Fi] = g[N,Fo] . ws[s][Fo,Fi]   (s = 0..nseg-1),
 * with g optionally masked by the ReLU of the forward output (`out_for_mask`:
 * g is taken as 0 where out <= 0; NULL = no mask). */
int dc_tag_linear_bwd_dx(const float *g, int64_t ldg, const float *out_for_mask, int64_t ldo,
                         const float *const *ws, int nseg, float *const *gxs,
                         DC_HOST const int64_t *ldgxs, int64_t N, int64_t Fi, int64_t Fo,
                         dc_stream_t stream);

/* Variants on the bf16 matrix cores.  Every fp32 operand is split exactly into bf16 terms
 * (hi + mid + lo) while it is staged into LDS and a product tile is `products`
 * v_mfma_f32_32x32x16_bf16 with fp32 accumulation:
 *   products = 6 : hi*hi, hi*mid, mid*hi, hi*lo, lo*hi, mid*mid - fp32-accurate (split error
 *                  ~6e-9 relative, below the rounding of the fp32 accumulation), 2.7x the
 *                  fp32 MFMA peak;
 *   products = 3 : hi*hi, hi*mid, mid*hi (~4e-6 relative);
 *   products = 1 : plain bf16 operands, fp32 accumulate (BASELINE.json configs[4]).
 * Same arguments and semantics as the functions above; shapes the split kernels do not cover
 * (unaligned operands, reduction extent not a multiple of 16) silently take the fp32 path.
 * The dX variant needs a scratch of ..._workspace_bytes() for transposed weights. */
int dc_tag_linear_fwd_split(const float *const *xs, DC_HOST const int64_t *ldxs, const float *const *ws,
                            int nseg, const float *bias, int relu, float *out, int64_t ldo,
                            int64_t N, int64_t Fi, int64_t Fo, int products, dc_stream_t stream);
/* The forward dense block of a TAGConv layer with a SHORT reduction - the first layer of each encoder branch
 * (/root/reference/models/model.py:44-50: TAGConv(21, 256), TAGConv(25, 256); PyG tag_conv.py: sum_k lins[k](x_k) + bias,
 * followed by the F.relu of models/model.py:71,77):
 *     out[N, 256] = act(slab[N, wpad] . [W_0 | ... | W_{nseg-1} | 0]^T + bias)
 * slab = the layer's hop slab, (nseg * fi) data columns zero-padded to wpad = 96 / 112 / 128; ws[k] = lins[k].weight
 * [256, fi], read as they are (no packing launch).  Six-product bf16 arithmetic, bit-identical to dc_tag_linear_fwd_split
 * (products = 6) on the packed weights.  One persistent launch, weights resident in registers, whole reduction in one
 * stage, 1-KiB row stores (dc_dense_narrow.hip).  _ok: host-side query whether the entry takes a shape. */
int dc_tag_linear_fwd_narrow_ok(int64_t fi, int nseg, int64_t wpad, int64_t Fo);
int dc_tag_linear_fwd_narrow(const float *slab, int64_t ld, const float *const *ws, int nseg, int64_t fi,
                             const float *bias, int relu, float *out, int64_t ldo, int64_t N, int64_t wpad,
                             int64_t Fo, dc_stream_t stream);
/* The same block on PREPARED weights.  dc_tag_narrow_wimage: wimg (wpad / 16 * 24576 bytes, 16-byte aligned) = the three
 * bf16 planes (hi, mid, lo: round-to-nearest-even of x, x - hi, x - hi - mid) of [W_0 | ... | W_{nseg-1} | 0] in the order
 * the kernel's lanes hold them: [wpad / 16 k-steps][3 planes][8 column blocks of 32][64 lanes][8 bf16], record
 * (ks, plane, block, lane = c + 32 h) = columns k = 16 ks + 8 h .. + 7 of output column 32 block + c.  ws[k] may sit at
 * any 4-byte-aligned address.  dc_tag_linear_fwd_narrow_img: the forward block reading that image - no weight prologue
 * per workgroup, two workgroups per CU for wpad = 96 / 112; outputs bit-identical to dc_tag_linear_fwd_narrow. */
int dc_tag_narrow_wimage(const float *const *ws, int nseg, int64_t fi, int64_t wpad, void *wimg, dc_stream_t stream);
int dc_tag_linear_fwd_narrow_img(const float *slab, int64_t ld, const void *wimg, const float *bias, int relu,
                                 float *out, int64_t ldo, int64_t N, int64_t wpad, int64_t Fo, dc_stream_t stream);
int64_t dc_tag_linear_bwd_dx_split_workspace_bytes(int64_t Fi, int64_t Fo, int nseg);
int dc_tag_linear_bwd_dx_split(const float *g, int64_t ldg, const float *out_for_mask,
                               int64_t ldo, const float *const *ws, int nseg, float *const *gxs,
                               DC_HOST const int64_t *ldgxs, void *workspace, int64_t workspace_bytes,
                               int64_t N, int64_t Fi, int64_t Fo, int products, dc_stream_t stream);

/* dW-side: (g*relu')^T[Fo,N] . xs[s][N,Fi] (same optional ReLU mask), gbias[Fo] = column
 * sums of g*relu' (NULL to skip).  The result is delivered as `ngw` output blocks (ngw a
 * multiple of nseg): block j = columns [(j % bps)*gw_cols, +gw_cols) of segment j / bps,
 * bps = ngw / nseg, written to gws[j] as a contiguous [Fo, gw_cols] matrix - i.e. one block
 * per PyG `lins[k].weight` whether the layer ran as K+1 segments (ngw = nseg, gw_cols = Fi)
 * or as one concatenated segment (nseg = 1, ngw = K+1, gw_cols = F_in).  accumulate != 0 adds
 * into gws / gbias (fused gradient accumulation) instead of overwriting.
 * `partials` is a caller-owned scratch of dc_tag_linear_bwd_dw_workspace_bytes() bytes
 * (split-N partial slabs, summed in chunk order by a second kernel: deterministic, no float
 * atomics). */
int64_t dc_tag_linear_bwd_dw_workspace_bytes(int64_t N, int64_t Fi, int64_t Fo, int nseg);
int dc_tag_linear_bwd_dw(const float *g, int64_t ldg, const float *out_for_mask, int64_t ldo,
                         const float *const *xs, DC_HOST const int64_t *ldxs, int nseg,
                         float *const *gws, int ngw, int64_t gw_cols, float *gbias,
                         int accumulate, void *partials, int64_t partials_bytes, int64_t N,
                         int64_t Fi, int64_t Fo, dc_stream_t stream);
/* split-bf16x6 variant of the above (operands read through ds_read_b64_tr_b16) */
int dc_tag_linear_bwd_dw_split(const float *g, int64_t ldg, const float *out_for_mask,
                               int64_t ldo, const float *const *xs, DC_HOST const int64_t *ldxs, int nseg,
                               float *const *gws, int ngw, int64_t gw_cols, float *gbias,
                               int accumulate, void *partials, int64_t partials_bytes, int64_t N,
                               int64_t Fi, int64_t Fo, int products, dc_stream_t stream);

/* ---- fp16x2 ("h2") dense block: two scaled fp16 planes per operand, 3 MFMA products ---------
 * Same results contract as the *_split entries with products = 6 (fp32-accurate: simulated and
 * measured error at the level of fp32 accumulation) at half the matrix work.  Every operand is
 * multiplied by an exact power of two that puts its reference magnitude in [2^14, 2^15) before it
 * is written as h1 + h2 (fp16), and the accumulator is multiplied back:
 *   forward : row i of x by x_rowmax[i] >= max_k |x_k[i,:]| (dc_spmm_f32_rowmax records it for
 *             free), row o of the weights by w_rowmax[o] = max_s,f |W_s[o,f]| (dc_tag_weight_rowmax);
 *   dX      : row i of g * relu' by g_rowmax[i] >= max |g[i,:]| (dc_rowabsmax_f32), all weights by
 *             max_o w_rowmax[o] (reduced inside the kernel);
 *   dW      : the contraction runs over nodes, so g * relu' and x get ONE scale per node chunk of
 *             the split-N plan: the maxima of g_rowmax / x_rowmax over the chunk (inside the kernel).
 * Any upper bound is a valid reference.  fp16 denormals are honoured by the matrix core: elements
 * down to 2^-39 of their reference keep absolute accuracy.  The shared-scale entries (dX: the
 * weights, dW: a node chunk) are therefore fp32-accurate only while rows that meet in one reduction
 * spread over at most 2^22 against each other (gradient rows falling while activation rows rise;
 * table in DESIGN.md 4.3).  Shapes: Fi % 16 == 0 (forward),
 * Fo % 16 == 0 (dX), N % 16 == 0 (dW), 16-byte aligned rows; otherwise DC_EINVAL (use *_split). */
int dc_tag_linear_fwd_h2(const float *const *xs, DC_HOST const int64_t *ldxs, const float *const *ws,
                         int nseg, const float *bias, int relu, float *out, int64_t ldo, int64_t N,
                         int64_t Fi, int64_t Fo, const float *x_rowmax, const float *w_rowmax,
                         dc_stream_t stream);
int dc_tag_linear_bwd_dx_h2(const float *g, int64_t ldg, const float *out_for_mask, int64_t ldo,
                            const float *const *ws, int nseg, float *const *gxs,
                            DC_HOST const int64_t *ldgxs, void *workspace, int64_t workspace_bytes,
                            int64_t N, int64_t Fi, int64_t Fo, const float *g_rowmax,
                            const float *w_rowmax, dc_stream_t stream);
int dc_tag_linear_bwd_dw_h2(const float *g, int64_t ldg, const float *out_for_mask, int64_t ldo,
                            const float *const *xs, DC_HOST const int64_t *ldxs, int nseg,
                            float *const *gws, int ngw, int64_t gw_cols, float *gbias,
                            int accumulate, void *partials, int64_t partials_bytes, int64_t N,
                            int64_t Fi, int64_t Fo, const float *g_rowmax, const float *x_rowmax,
                            dc_stream_t stream);
/* dc_tag_linear_bwd_dw_h2 (no mask, no bias) with the gradient operand g[i, :] - g2_coef[i] * g2[i, :] formed at load
 * time (g2 with g's leading dimension): the attention backward's dK = (dS' - eps o P)^T Q without materialising the
 * corrected dS.  128 x 256 tile kernel only: Fo % 128 == 0, Fi == 256 per segment, N % 32 == 0. */
int dc_tag_linear_bwd_dw_h2_corr(const float *g, int64_t ldg, const float *g2, const float *g2_coef,
                                 const float *const *xs, DC_HOST const int64_t *ldxs, int nseg, float *const *gws, int ngw,
                                 int64_t gw_cols, int accumulate, void *partials, int64_t partials_bytes, int64_t N,
                                 int64_t Fi, int64_t Fo, const float *g_rowmax, const float *x_rowmax,
                                 dc_stream_t stream);
/* Backward in the forward's shape (used with the h2 entries):  the input gradient of a TAGConv layer
 *   gx = sum_k (A^T)^k (gm W_k),  gm = g * relu'
 * equals  sum_k ((A^T)^k gm) W_k  (A acts on rows, W_k on columns), i.e. K transposed hops on gm
 * followed by ONE dense block with the K = (K+1)*Fo reduction of the forward: dc_tag_linear_fwd_h2
 * over the hop slab of gm with the transposed weights.  Helpers:
 *   dc_tag_mask_grad         gm[i,:] = g[i,:] * (out_for_mask[i,:] > 0) into (a column block of) the
 *                            slab, rowmax_a[i] = rowmax_b[i] = max |gm[i,:]| (rowmax_b may be NULL);
 *   dc_tag_transpose_weights wt[s] [Fi, Fo] = ws[s]^T, s < nseg, packed back to back. */
int dc_tag_mask_grad(const float *g, int64_t ldg, const float *out_for_mask, int64_t ldo, float *gm,
                     int64_t ldgm, int64_t N, int64_t F, float *rowmax_a, float *rowmax_b,
                     dc_stream_t stream);
int dc_tag_transpose_weights(const float *const *ws, int nseg, int64_t Fo, int64_t Fi, float *wt,
                             dc_stream_t stream);
/* One launch for everything the h2 blocks of a layer need from its weights W_s [Fo, Fi], s < nseg:
 *   w_rowmax [Fo]          as dc_tag_weight_rowmax;
 *   w_image                (optional) the weights ALREADY scaled and split for the forward block: for
 *                          row o and every 16-wide stage of the concatenated reduction k = s*Fi + f one
 *                          64-byte record {h1[16], h2[16]} (fp16), W*2^e(o) = h1 + h2 with the row's scale
 *                          - Fo * nseg*Fi * 4 bytes, 16-byte aligned; consumed by dc_tag_linear_fwd_h2p,
 *                          which moves it global -> LDS by LDS-DMA instead of re-splitting the weights in
 *                          every row tile;
 *   wt_image, wt_rowmax    (optional, together) the same for the transposed weights (row f, reduction
 *                          k = s*Fo + o, wt_rowmax[f] = max_s,o |W_s[o,f]| [Fi]) for the forward-shaped
 *                          backward block. */
int dc_tag_weight_prep(const float *const *ws, int nseg, int64_t Fo, int64_t Fi, float *w_rowmax,
                       void *w_image, void *wt_image, float *wt_rowmax, dc_stream_t stream);
/* dc_tag_weight_prep that ALSO clears zero[0:zero_n] (fp32) in the same launch: the row-maxima buffer the layer's
 * dc_hop_chain_f32 launch joins its maxima into (mode | 2) - a separate memset node costs ~5 us on the critical path
 * of every forward chain. */
int dc_tag_weight_prep_zero(const float *const *ws, int nseg, int64_t Fo, int64_t Fi, float *w_rowmax,
                            void *w_image, void *wt_image, float *wt_rowmax, float *zero, int64_t zero_n,
                            dc_stream_t stream);
/* dc_tag_linear_fwd_h2 for ONE segment x [N, K] (ldx) with pre-split weights (w_image of
 * dc_tag_weight_prep; K = nseg*Fi of that call): out = act(x . W^T + b).  With a workspace of
 * dc_tag_linear_fwd_h2p_workspace_bytes (may be NULL / 0) a long reduction with too few output
 * tiles for the chip (no bias, no relu, ldo == Fo) is cut into ranges whose partials are summed in
 * range order by a second launch (deterministic). */
int64_t dc_tag_linear_fwd_h2p_workspace_bytes(int64_t N, int64_t K, int64_t Fo);
int dc_tag_linear_fwd_h2p(const float *x, int64_t ldx, const void *w_image, const float *bias, int relu,
                          float *out, int64_t ldo, int64_t N, int64_t K, int64_t Fo,
                          const float *x_rowmax, const float *w_rowmax, void *workspace,
                          int64_t workspace_bytes, dc_stream_t stream);
/* The attention backward's recompute of a block's softmax weights in ONE launch (models/model.py:15-17 as the
 * blocked form evaluates it): out[i, j] = exp(x[i,:] . W[j,:] - row_lse[i]) for j < ncols_valid, 0 for the padded
 * columns ncols_valid <= j < Fo - dc_tag_linear_fwd_h2p (no bias, no relu) with dc_attn_exp_rows applied in the
 * epilogue; bit-identical to the two launches. */
int dc_tag_linear_fwd_h2p_exp(const float *x, int64_t ldx, const void *w_image, float *out, int64_t ldo,
                              int64_t N, int64_t K, int64_t Fo, const float *x_rowmax, const float *w_rowmax,
                              const float *row_lse, int64_t ncols_valid, dc_stream_t stream);
/* dc_tag_linear_fwd_h2p (no bias, no relu, no split reduction) with the left operand x[i, :] - x2_coef[i] * x2[i, :]
 * formed at load time (x2 with x's leading dimension): the attention backward's dQ = (dS' - eps o P) K without
 * materialising the corrected dS.  128 x 256 tile kernel only (K % 32 == 0, 16-byte aligned rows). */
int dc_tag_linear_fwd_h2p_corr(const float *x, int64_t ldx, const float *x2, const float *x2_coef, const void *w_image,
                               float *out, int64_t ldo, int64_t N, int64_t K, int64_t Fo, const float *x_rowmax,
                               const float *w_rowmax, dc_stream_t stream);
/* ---- grouped launches: both encoder branches as ONE block-diagonal launch ----
 * The reference runs its two branches as 2 x 2 conv calls (models/model.py:69-78).  Over a merged node
 * space (dc_graph_build_parts) the second layers of both branches - same widths, different weights -
 * become single launches: the hops need nothing new (one adjacency), the dense blocks take GROUPS:
 * group g = rows [row_beg[g], row_beg[g] + rows[g]) of the merged matrices, with its own weights.
 * row_beg[g] and N_total are multiples of DC_GROUP_ALIGN; the rows between groups are padding the
 * CALLER keeps at zero in x and in the gradients (isolated nodes: the hops write zeros there), so
 * they add exact zeros to dW and their outputs are never read.  Per row the arithmetic is exactly
 * that of the ungrouped h2 entries on that group alone: outputs, dX and (with the per-group node
 * chunks of the ungrouped plan) dW are bit-identical to separate launches.
 *   dc_tag_grouped_weight_prep   dc_tag_weight_prep for every group in one launch; ws[g*nseg + s],
 *                                per-group output pointer arrays [ngroups]
 *   dc_tag_grouped_fwd_h2p       dc_tag_linear_fwd_h2p (K % 32 == 0; forward and, with the transposed
 *                                images over the gradient slab, dX)
 *   dc_tag_grouped_mask_grad     dc_tag_mask_grad with one upstream-gradient matrix per group
 *                                (g[k] = rows[k] x F, local row numbering); padding rows get zeros
 *   dc_tag_grouped_bwd_dw_h2     dc_tag_linear_bwd_dw_h2 on the pre-masked gradient (Fi == 256 per
 *                                segment, Fo % 128 == 0): gws[g*nseg + s] [Fo, Fi], gbias[g] [Fo] */
int dc_tag_grouped_weight_prep(const float *const *ws, int ngroups, int nseg, int64_t Fo, int64_t Fi,
                               float *const *w_rowmax, void *const *w_image, void *const *wt_image,
                               float *const *wt_rowmax, dc_stream_t stream);
int dc_tag_grouped_fwd_h2p(const float *x, int64_t ldx, int ngroups, DC_HOST const int64_t *row_beg,
                           DC_HOST const int64_t *rows, int64_t N_total, const void *const *w_images,
                           const float *const *biases, int relu, float *out, int64_t ldo, int64_t K,
                           int64_t Fo, const float *x_rowmax, const float *const *w_rowmaxes,
                           dc_stream_t stream);
int dc_tag_grouped_mask_grad(const float *const *g, DC_HOST const int64_t *ldg, int ngroups,
                             DC_HOST const int64_t *row_beg, DC_HOST const int64_t *rows, int64_t N_total,
                             const float *out_for_mask, int64_t ldo,
                             float *gm, int64_t ldgm, int64_t F, float *rowmax_a, float *rowmax_b,
                             dc_stream_t stream);
int64_t dc_tag_grouped_bwd_dw_workspace_bytes(DC_HOST const int64_t *rows, int ngroups, int64_t Fi, int64_t Fo,
                                              int nseg);
int dc_tag_grouped_bwd_dw_h2(const float *g, int64_t ldg, const float *const *xs, DC_HOST const int64_t *ldxs,
                             int nseg, int ngroups, DC_HOST const int64_t *row_beg, DC_HOST const int64_t *rows,
                             int64_t N_total, float *const *gws, float *const *gbias, int accumulate,
                             void *partials, int64_t partials_bytes, int64_t Fi, int64_t Fo,
                             const float *g_rowmax, const float *x_rowmax, dc_stream_t stream);

/* Number of launches of the GENERIC dense kernels (any shape / alignment, bounds logic per load, scalar
 * loads when misaligned) since the library was loaded or the counter was last reset (reset != 0 returns the
 * count and clears it).  Every shape of the shipped configuration has a tuned kernel; a non-zero count after a
 * default-config step means an operand lost its alignment or a shape fell off the fast paths (round 2 found two
 * such silent fallbacks only through DC_DENSE_TRACE=1) - the test suite pins it at zero. */
int64_t dc_generic_dense_launches(int reset);

/* Launch log: which kernels does a step actually launch?  dc_kernel_trace(1) clears the log and starts counting every
 * kernel launch of the library by kernel name as written at its launch site (e.g. "k_fwd_h2w<true, false>"; template
 * parameters of the launching host function stay symbolic: "k_hop_chain_gcn<STEPS>"), dc_kernel_trace(0) stops.
 * dc_kernel_trace_dump writes "name count\n" lines into buf (NUL-terminated, truncated to cap bytes) and returns the
 * size the whole text needs.  Process-wide, thread-safe, off by default (one predictable branch per launch). */
void dc_kernel_trace(int on);
int64_t dc_kernel_trace_dump(char *buf, int64_t cap);

/* Launch sites: the library lists its own kernel launches.  Every launch in the sources leaves one static record in
 * the library's data (host code only: the list needs no GPU); a templated host launcher leaves one per instantiation.
 * A site's identity is "kernel text @ enclosing host function", the kernel text as in the launch log, the function as
 * the compiler prints it with its template arguments, e.g.
 *     k_hop_chain<true, 3, 8> @ bool dc::launch_chain_steps(...) [W = true, STEPS = 3, LPR = 8]
 * (a second launch of the same kernel text in one function gets " #2").
 * dc_launch_sites_dump writes one "source file\tidentity\n" line per site.  dc_launch_coverage(1) starts, (0) stops
 * adding every site that launches to a cumulative reached set, which is never cleared and is independent of
 * dc_kernel_trace; dc_launch_reached_dump writes one "identity\ttest\tlaunches\n" line per reached site, `test` being
 * the environment's PYTEST_CURRENT_TEST at the site's first launch (empty when unset) and `launches` the site's launches
 * while coverage was on (its difference around a call names exactly the sites that call launched).  Both dumps fill buf like
 * dc_kernel_trace_dump and return the size the whole text needs.  Off by default, at no cost beyond the launch
 * log's one predictable branch. */
int64_t dc_launch_sites_dump(char *buf, int64_t cap);
void dc_launch_coverage(int on);
int64_t dc_launch_reached_dump(char *buf, int64_t cap);

/* rowmax[i] = max |x[i, 0:F]| for a row-major [N, F] view with leading dimension ld. */
int dc_rowabsmax_f32(const float *x, int64_t ld, int64_t N, int64_t F, float *rowmax,
                     dc_stream_t stream);
/* w_rowmax[o] = max over the nseg weight blocks W_s [Fo, Fi] and f of |W_s[o, f]|. */
int dc_tag_weight_rowmax(const float *const *ws, int nseg, int64_t Fo, int64_t Fi, float *w_rowmax,
                         dc_stream_t stream);

/* pos_of[perm[p]] = p  (inverse permutation over the E' = *ptr_last sorted edges) */
int dc_invert_perm(const int32_t *perm, const int32_t *ptr_last /* &ptr[N] */, int32_t *pos_of,
                   int64_t max_edges, dc_stream_t stream);
/* out[p] = a[b[p]] for p < *count_ptr (e.g. position-in-forward-order of every
 * backward-ordered edge: a = pos_of, b = perm of the key_row=0 set). */
int dc_compose_perm(const int32_t *a, const int32_t *b, int32_t *out, const int32_t *count_ptr,
                    int64_t cap, dc_stream_t stream);

/* ---- GCNConv / GATConv: the row-wise passes around the aggregation, fused (dc_gnn_epi.hip) ----
 * PyG gcn_conv.py / gat_conv.py: out = propagate(...) + bias; the encoder loop then applies relu
 * (models/model.py:71,77); GAT: alpha_src = (h * att_src).sum(-1), alpha_dst likewise.
 *   dc_spmm_f32_bias_act : y[i,:] = act(sum_p w[p] x[other[p],:] + bias)  (bias may be NULL, relu 0/1);
 *                          the sum as dc_spmm_f32, bias added to the finished sum: same values as the
 *                          three separate passes
 *   dc_mask_colsum_f32   : gm = g * (y_mask > 0) (y_mask NULL: gm = g; gm NULL: not written) and
 *                          colsum[c] (+)= sum_i gm[i,c] (the bias gradient), per-block partials combined
 *                          in block order - deterministic; workspace of dc_colsum_workspace_bytes(N,F,1)
 *   dc_gat_alpha_fwd     : a_src[i] = h[i,:] . att_src, a_dst[i] = h[i,:] . att_dst, one pass over h
 *   dc_gat_alpha_bwd     : gh[i,:] += ga_src[i] att_src + ga_dst[i] att_dst (gh holds the aggregation's
 *                          gradient), g_att_src (+)= sum_i ga_src[i] h[i,:], g_att_dst likewise; workspace
 *                          of dc_colsum_workspace_bytes(N,F,2)
 * F % 4 == 0 and 16-byte aligned rows; the column-sum passes need F/4 to divide 256. */
int dc_spmm_f32_bias_act(const int32_t *ptr, const int32_t *other, const float *w, const float *x,
                         int64_t ldx, const float *bias, int relu, float *y, int64_t ldy, int64_t N,
                         int64_t F, dc_stream_t stream);
int64_t dc_colsum_workspace_bytes(int64_t N, int64_t F, int nvec);
int dc_mask_colsum_f32(const float *g, int64_t ldg, const float *y_mask, int64_t ldy, float *gm,
                       int64_t ldgm, int64_t N, int64_t F, void *workspace, int64_t workspace_bytes,
                       float *colsum, int accumulate, dc_stream_t stream);
int dc_gat_alpha_fwd(const float *h, int64_t ldh, const float *att_src, const float *att_dst, float *a_src,
                     float *a_dst, int64_t N, int64_t F, dc_stream_t stream);
int dc_gat_alpha_bwd(const float *h, int64_t ldh, const float *ga_src, const float *ga_dst,
                     const float *att_src, const float *att_dst, float *gh, int64_t ldgh, int64_t N,
                     int64_t F, void *workspace, int64_t workspace_bytes, float *g_att_src,
                     float *g_att_dst, int accumulate, dc_stream_t stream);

/* ---- GATConv edge terms (nn/conv/gat_conv.py edge_update + utils/_softmax.py) -
 * Only reached when the reference is configured with backbone "GATConv"
 * (models/model.py:39).  Arrays are in key_row=1 order of a self_loops=1 set;
 * segments = incoming edges of node i.
 *   e_p     = leaky_relu(a_src[other[p]] + a_dst[i], slope)
 *   alpha_p = exp(e_p - max_seg e) / (sum_seg exp(e - max) + 1e-16)
 * The aggregation out_i = sum_p alpha_p h[other[p]] is dc_spmm_f32 with w = alpha.
 */
int dc_gat_edge_softmax_fwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                            const float *a_dst, float slope, float *alpha, int64_t N,
                            dc_stream_t stream);
/* Backward: given galpha[E'] writes ge[p] = d loss / d (a_src[other[p]] + a_dst[i])
 * (softmax and leaky-relu chained) and g_a_dst[i] = sum of ge over segment i. */
int dc_gat_edge_softmax_bwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                            const float *a_dst, float slope, const float *alpha,
                            const float *galpha, float *ge, float *g_a_dst, int64_t N,
                            dc_stream_t stream);
/* Sampled dense-dense product: d[p] = <g[i,0:F], h[other[p],0:F]> for p in segment i
 * (gradient of the aggregation w.r.t. alpha). */
int dc_sddmm_f32(const int32_t *ptr, const int32_t *other, const float *g, int64_t ldg,
                 const float *h, int64_t ldh, float *d, int64_t N, int64_t F,
                 dc_stream_t stream);
/* out[i] = sum over p in [ptr[i],ptr[i+1]) of v[map ? map[p] : p]  (p order) */
int dc_segment_sum_f32(const int32_t *ptr, const int32_t *map, const float *v, float *out,
                       int64_t N, dc_stream_t stream);
/* out[p] = v[idx[p]] for p < *count_ptr */
int dc_gather_f32(const float *v, const int32_t *idx, float *out, const int32_t *count_ptr,
                  int64_t cap, dc_stream_t stream);

/* ---- GATConv with H attention heads (heads > 1; concat or mean over heads) (dc_gat_heads.hip) ----
 * PyG gat_conv.py with h = lin(x) viewed as [N, H, C].  The entries above carry one scalar per edge and
 * per node; these carry H, EDGE-MAJOR: a_src / a_dst / g_a_src / g_a_dst are [N, H] row-major, alpha /
 * galpha / ge are [capacity, H] in key_row=1 order - the H values of an edge sit together, so one read
 * of other[p] and of the segment bounds serves every head and a neighbour row of H*C floats is gathered
 * once.  Any H >= 1, C >= 1 and in-degree; sums in p order, no float atomics (deterministic).
 *   dc_gat_alpha_heads_fwd        : a_src[i,k] = h[i,kC:(k+1)C] . att_src[kC:(k+1)C], a_dst likewise (att_*
 *                                   are the [1,H,C] parameters, flat), one pass over h
 *   dc_gat_edge_softmax_heads_fwd : alpha[p,k] = softmax over segment i of leaky_relu(a_src[other[p],k] +
 *                                   a_dst[i,k]), denominator + 1e-16; per head the arithmetic of
 *                                   dc_gat_edge_softmax_fwd
 *   dc_spmm_f32_heads_bias_act    : y[i,c] = act(sum_p alpha[p,c/C] x[other[p],c] + bias[c]) over the H*C
 *                                   columns; mean != 0: y[i,c] = act((sum_k sum_p alpha[p,k] x[other[p],kC+c]) / H
 *                                   + bias[c]) over C columns.  Sum from zero in p order, bias added to the
 *                                   finished sum (bias may be NULL, relu 0/1); 16-byte loads when C % 4 == 0
 *                                   and rows are 16-byte aligned.  On the key_row=0 set with alpha re-ordered by
 *                                   source (dc_gather_f32_heads) it is the transposed aggregation of the backward.
 *   dc_sddmm_f32_heads            : d[p,k] = <g[i,kC:(k+1)C], h[other[p],kC:(k+1)C]>, each h row read once
 *   dc_gat_edge_softmax_heads_bwd : ge[p,k] and g_a_dst[i,k] = sum over segment i of ge[p,k], as
 *                                   dc_gat_edge_softmax_bwd per head
 *   dc_segment_sum_f32_heads      : out[i,k] = sum over p in segment i of v[map ? map[p] : p, k], rows of W floats
 *   dc_gather_f32_heads           : out[p,:] = v[idx[p],:] for p < *count_ptr, rows of W floats
 *   dc_spread_heads_f32           : out[i,kC+c] = g[i,c] / H (the gradient of the mean over heads)
 *   dc_gat_alpha_heads_bwd        : gh[i,c] += ga_src[i,c/C] att_src[c] + ga_dst[i,c/C] att_dst[c], g_att_src[c]
 *                                   (+)= sum_i ga_src[i,c/C] h[i,c], g_att_dst likewise, per-block partials
 *                                   combined in block order; H*C % 4 == 0 with H*C/4 dividing 256, 16-byte
 *                                   aligned rows, workspace of dc_colsum_workspace_bytes(N, H*C, 2) */
int dc_gat_alpha_heads_fwd(const float *h, int64_t ldh, const float *att_src, const float *att_dst,
                           float *a_src, float *a_dst, int64_t N, int64_t H, int64_t C, dc_stream_t stream);
int dc_gat_edge_softmax_heads_fwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                                  const float *a_dst, float slope, float *alpha, int64_t N, int64_t H,
                                  dc_stream_t stream);
int dc_spmm_f32_heads_bias_act(const int32_t *ptr, const int32_t *other, const float *alpha, const float *x,
                               int64_t ldx, const float *bias, int relu, int mean, float *y, int64_t ldy,
                               int64_t N, int64_t H, int64_t C, dc_stream_t stream);
int dc_sddmm_f32_heads(const int32_t *ptr, const int32_t *other, const float *g, int64_t ldg, const float *h,
                       int64_t ldh, float *d, int64_t N, int64_t H, int64_t C, dc_stream_t stream);
int dc_gat_edge_softmax_heads_bwd(const int32_t *ptr, const int32_t *other, const float *a_src,
                                  const float *a_dst, float slope, const float *alpha, const float *galpha,
                                  float *ge, float *g_a_dst, int64_t N, int64_t H, dc_stream_t stream);
int dc_segment_sum_f32_heads(const int32_t *ptr, const int32_t *map, const float *v, float *out, int64_t N,
                             int64_t W, dc_stream_t stream);
int dc_gather_f32_heads(const float *v, const int32_t *idx, float *out, const int32_t *count_ptr, int64_t cap,
                        int64_t W, dc_stream_t stream);
int dc_spread_heads_f32(const float *g, int64_t ldg, float *out, int64_t ldo, int64_t N, int64_t H, int64_t C,
                        dc_stream_t stream);
int dc_gat_alpha_heads_bwd(const float *h, int64_t ldh, const float *ga_src, const float *ga_dst,
                           const float *att_src, const float *att_dst, float *gh, int64_t ldgh, int64_t N,
                           int64_t H, int64_t C, void *workspace, int64_t workspace_bytes, float *g_att_src,
                           float *g_att_dst, int accumulate, dc_stream_t stream);

/* ---- GATConv edge features (edge_dim = D, edge_attr [E, D]) (dc_gat_edge.hip, dc_gat_heads.hip) ----
 * PyG gat_conv.py with edge_attr: the logit of edge p into i from j and head k is
 *   leaky_relu((a_src[j,k] + a_dst[i,k]) + a_edge[p,k]),  a_edge[p,k] = <lin_edge(edge_attr[p])[k,:], att_edge[k,:]>
 * added in that order (an a_edge of zeros leaves every bit of the entries above).  The term is linear in edge_attr:
 * a_edge[p,:] = attr[p,:] @ M with the caller's folded M [D, H] row-major, M[d,k] = sum_c lin_edge.weight[kC+c,d]
 * att_edge[k,c]; [E, H*C] is never formed.  Arrays are in key_row=1 order of a self_loops=1 set (ptr / perm of
 * dc_graph_build): sorted edge p is input edge perm[p] < E - row perm[p] of edge_attr, float32, row stride lda >= D,
 * inner stride 1 - or the appended loop of node perm[p] - E, whose attribute row is fill_value: fill_mean != 0 the mean
 * of the attribute rows of the other edges into the node, summed in p order from zero and divided by their count (0
 * where there are none), else the constant fill_value in every component.  Input self loops were dropped by the build
 * and appear nowhere.  1 <= D <= DC_GAT_EDGE_MAX_DIM, any H >= 1 and in-degree, E = 0 (edge_attr may be NULL), N = 1;
 * sums in fixed order, no float atomics (deterministic).
 *   dc_gat_edge_attr_fwd         : a_edge [capacity, H] edge-major (rows ptr[N].. untouched), sum over d in d order;
 *                                  loop_attr [N, D] = the attribute row of every node's appended loop
 *   dc_gat_edge_attr_softmax_fwd : dc_gat_edge_softmax_heads_fwd with the addend (same kernel template)
 *   dc_gat_edge_attr_softmax_bwd : dc_gat_edge_softmax_heads_bwd with the addend: the leaky-relu derivative looks at
 *                                  the full logit; ge is the gradient of the pre-activation logit, hence of a_edge
 *   dc_gat_edge_attr_bwd         : g_edge_attr (NULL: skipped) [E, D], row stride ldg: row perm[p] =
 *                                  (ge[p,:] + ge[loop of i,:] / cnt_i) @ M^T with fill_mean, ge[p,:] @ M^T without -
 *                                  every input edge written by one thread, rows of dropped input self loops zero;
 *                                  g_m (NULL: skipped) [D, H]: g_m[d,k] = sum_p attr[p,d] ge[p,k] over all sorted
 *                                  edges p < ptr[N] (loops with loop_attr), per-workgroup partials of 1,024 edges in
 *                                  the workspace (dc_gat_edge_attr_bwd_workspace_bytes(capacity, D, H)) combined in
 *                                  workgroup order.  capacity = rows of ge (E + N). */
#define DC_GAT_EDGE_MAX_DIM 64
int dc_gat_edge_attr_fwd(const int32_t *ptr, const int32_t *perm, const float *edge_attr, int64_t lda, const float *m,
                         int fill_mean, float fill_value, float *a_edge, float *loop_attr, int64_t N, int64_t E,
                         int64_t D, int64_t H, dc_stream_t stream);
int dc_gat_edge_attr_softmax_fwd(const int32_t *ptr, const int32_t *other, const float *a_src, const float *a_dst,
                                 const float *a_edge, float slope, float *alpha, int64_t N, int64_t H,
                                 dc_stream_t stream);
int dc_gat_edge_attr_softmax_bwd(const int32_t *ptr, const int32_t *other, const float *a_src, const float *a_dst,
                                 const float *a_edge, float slope, const float *alpha, const float *galpha, float *ge,
                                 float *g_a_dst, int64_t N, int64_t H, dc_stream_t stream);
int64_t dc_gat_edge_attr_bwd_workspace_bytes(int64_t capacity, int64_t D, int64_t H);
int dc_gat_edge_attr_bwd(const int32_t *ptr, const int32_t *perm, const float *ge, const float *edge_attr, int64_t lda,
                         const float *loop_attr, const float *m, int fill_mean, float *g_edge_attr, int64_t ldg,
                         float *g_m, int64_t N, int64_t E, int64_t D, int64_t H, int64_t capacity, void *workspace,
                         int64_t workspace_bytes, dc_stream_t stream);

/* ---- GATv2Conv: dynamic attention (dc_gatv2.hip) ----
 * PyG gatv2_conv.py with xl = lin_l(x), xr = lin_r(x) viewed as [N, H, C] (row-major [N, H*C], row strides ld* >= H*C;
 * xl == xr with share_weights).  For sorted edge p from j = other[p] into i, head k, channel c:
 *   s[p,k,c] = xl[j,k,c] + xr[i,k,c],   e[p,k] = sum_c att[k,c] leaky_relu(s[p,k,c]),
 *   alpha[p,k] = softmax of e[.,k] over segment i (maximum subtracted, denominator + 1e-16)
 * att is the [1,H,C] parameter, flat.  alpha / galpha / ge are [capacity, H] edge-major in key_row=1 order, as for the
 * entries of dc_gat_heads.hip, whose dc_spmm_f32_heads_bias_act (aggregation of xl) and dc_sddmm_f32_heads (galpha[p,k] =
 * <gm[i,k,:], xl[j,k,:]>) the layer uses as they are.  Any H >= 1, C >= 1 and in-degree, N = 0; no width cap; 16-byte
 * loads when C % 4 == 0 and every row is 16-byte aligned.  Sums in a fixed order (the long ones compensated), no float
 * atomics: deterministic.  Arguments are checked before any HIP call, in this order in all three entries: sizes (N < 0,
 * H < 1, C < 1, range), leading dimensions, then null pointers - DC_EINVAL with the entry's name in dc_last_error().
 * N == 0 is the one exception to the null check: there is no row to read or write, so the per-row and per-edge arrays
 * may be NULL (an empty tensor has no address) and the call returns DC_OK; dc_gatv2_softmax_bwd still needs att and
 * g_att, which it writes (zeros, or g_att as it is with accumulate).
 *   dc_gatv2_softmax_fwd : alpha (rows ptr[N].. untouched); one wave per destination, xr[i] in registers, every xl[j]
 *                          element gathered once
 *   dc_gatv2_softmax_bwd : ge[p,k] = alpha[p,k] (galpha[p,k] - sum over segment i of alpha galpha), the gradient of e;
 *                          g_xr[i,k,c] = sum over the edges into i, in p order, of t[p,k,c] = ge[p,k] att[k,c]
 *                          (s[p,k,c] > 0 ? 1 : slope); g_att[k,c] (+)= sum_p ge[p,k] leaky_relu(s[p,k,c]): one row of
 *                          partial sums per workgroup of DC_GATV2_ROWS destinations in the workspace
 *                          (dc_gatv2_workspace_bytes(N, H, C)), added in workgroup order; accumulate != 0 adds to what
 *                          g_att holds
 *   dc_gatv2_source_bwd  : on the key_row=0 set (ptr_t / other_t; to_fwd[q] = position of transposed edge q in key_row=1
 *                          order): g_xl[j,k,c] = sum over the edges q out of j, in q order, of alpha[p,k] gm[i,k,c] +
 *                          t[p,k,c] with p = to_fwd[q], i = other_t[q] - both terms in one walk of the segment */
#define DC_GATV2_ROWS 32
int dc_gatv2_softmax_fwd(const int32_t *ptr, const int32_t *other, const float *xl, int64_t ldxl, const float *xr,
                         int64_t ldxr, const float *att, float slope, float *alpha, int64_t N, int64_t H, int64_t C,
                         dc_stream_t stream);
int64_t dc_gatv2_workspace_bytes(int64_t N, int64_t H, int64_t C);
int dc_gatv2_softmax_bwd(const int32_t *ptr, const int32_t *other, const float *alpha, const float *galpha,
                         const float *xl, int64_t ldxl, const float *xr, int64_t ldxr, const float *att, float slope,
                         float *ge, float *g_xr, int64_t ldg, float *g_att, int accumulate, void *workspace,
                         int64_t workspace_bytes, int64_t N, int64_t H, int64_t C, dc_stream_t stream);
int dc_gatv2_source_bwd(const int32_t *ptr_t, const int32_t *other_t, const int32_t *to_fwd, const float *alpha,
                        const float *ge, const float *gm, int64_t ldgm, const float *xl, int64_t ldxl, const float *xr,
                        int64_t ldxr, const float *att, float slope, float *g_xl, int64_t ldg, int64_t N, int64_t H,
                        int64_t C, dc_stream_t stream);

/* ---- TransformerConv: scaled dot-product edge attention (dc_transformer.hip) ----
 * PyG transformer_conv.py with q = lin_query(x), k = lin_key(x), v = lin_value(x) viewed as [N, H, C] (row-major
 * [N, H*C], row strides ld* >= H*C).  For sorted edge p from j = other[p] into i and head h:
 *   e[p,h] = (sum_c q[i,h,c] k[j,h,c]) * scale,   scale = float32(1 / sqrt(C)), given by the caller
 *   alpha[p,h] = softmax of e[.,h] over segment i (maximum subtracted, denominator + 1e-16)
 * alpha / galpha / gl are [capacity, H] edge-major in key_row=1 order, as for the entries of dc_gat_heads.hip, whose
 * dc_spmm_f32_heads_bias_act (aggregation of v) and dc_sddmm_f32_heads (galpha[p,h] = <gm[i,h,:], v[j,h,:]>) the layer
 * uses as they are.  The edge set is taken as given (no self loop is added): a row may have no edge.  Any H >= 1,
 * C >= 1 and in-degree >= 0, N = 0; no width cap, no workspace; 16-byte loads when C % 4 == 0 and every row is 16-byte
 * aligned.  Sums in a fixed order (the long ones compensated), no float atomics: deterministic.  Arguments are checked
 * before any HIP call, in this order in all three entries: sizes (N < 0, H < 1, C < 1, range), leading dimensions,
 * then null pointers - DC_EINVAL with the entry's name in dc_last_error().  N == 0 returns DC_OK before the null
 * check (an empty tensor has no address).
 *   dc_tconv_softmax_fwd : alpha (rows ptr[N].. untouched; nothing is written for a row without edges); one wave
 *                          per destination, q[i] in registers, every k[j] element gathered once; a segment's exp /
 *                          normalise passes are spread over the lanes of the head's group
 *   dc_tconv_softmax_bwd : gl[p,h] = alpha[p,h] (galpha[p,h] - sum over segment i of alpha galpha) * scale, the gradient
 *                          of <q_i, k_j>; g_q[i,h,c] = sum over the edges into i, in p order, of gl[p,h] k[j,h,c]
 *                          (zeros for a row without edges); one launch
 *   dc_tconv_source_bwd  : on the key_row=0 set (ptr_t / other_t; to_fwd[t] = position of transposed edge t in key_row=1
 *                          order), with p = to_fwd[t], i = other_t[t], sums over the edges t out of j in t order:
 *                          g_k[j,h,c] = sum gl[p,h] q[i,h,c] and g_v[j,h,c] = sum alpha[p,h] gm[i,h,c] - one walk */
int dc_tconv_softmax_fwd(const int32_t *ptr, const int32_t *other, const float *q, int64_t ldq, const float *k,
                         int64_t ldk, float scale, float *alpha, int64_t N, int64_t H, int64_t C, dc_stream_t stream);
int dc_tconv_softmax_bwd(const int32_t *ptr, const int32_t *other, const float *alpha, const float *galpha,
                         const float *k, int64_t ldk, float scale, float *gl, float *g_q, int64_t ldgq, int64_t N,
                         int64_t H, int64_t C, dc_stream_t stream);
int dc_tconv_source_bwd(const int32_t *ptr_t, const int32_t *other_t, const int32_t *to_fwd, const float *alpha,
                        const float *gl, const float *q, int64_t ldq, const float *gm, int64_t ldgm, float *g_k,
                        int64_t ldgk, float *g_v, int64_t ldgv, int64_t N, int64_t H, int64_t C, dc_stream_t stream);

/* ---- SAGEConv: mean and max over a node's in-edges (dc_sage.hip) ----
 * Segment reductions of x fp32 [N, F] (row strides ld* >= F) over the key_row=1 set (ptr / other = source ids) as it
 * is given - no self loop is added, duplicates count, a row may have no edge - and their backward over the key_row=0
 * set (ptr_t / other_t = destination ids).  Any F >= 1 (no width cap), any in-degree >= 0, N = 0; 16-byte loads when
 * F % 4 == 0 and every pointer and row stride is 16-byte aligned.  Sums in a fixed order (the backward sums
 * compensated), no float atomics, no workspace: deterministic.  Non-finite inputs: the
 * sums carry NaN / Inf into the rows and columns that depend on them and no others; the max forward selects among +-Inf
 * exactly and a NaN candidate makes m NaN with cnt = the number of NaN candidates; the backward of a non-finite forward
 * is not specified.
 * Arguments are checked before any HIP call, in this order: sizes (N < 0, F < 1, range), leading dimensions, then
 * null pointers, then aliasing - DC_EINVAL with the entry's name in dc_last_error().  N == 0 returns DC_OK before the
 * null check (an empty tensor has no address).
 *   dc_sage_mean_fwd : y[i,c] = (sum over the edges p into i, in p order, of x[other[p],c]) / float(ptr[i+1] - ptr[i])
 *                      - the plain fp32 sum of the unweighted dc_spmm_f32, then a true division; 0 for a row without
 *                      edges
 *   dc_sage_mean_bwd : gx[j,c] = sum over the edges t out of j, in t order, of gy[i,c] / float(in-degree of i),
 *                      i = other_t[t], the in-degree read from the key_row=1 ptr; one launch, no scaled copy of gy
 *   dc_sage_max_fwd  : m[i,c] = max over the edges into i of x[other[p],c]; cnt[i,c] (int32, NULL: not written) = the
 *                      number of those edges whose value equals it; a row without edges gives m = 0, cnt = 0
 *   dc_sage_max_bwd  : gx[j,c] = sum over the edges t out of j, in t order, of (x[j,c] == m[i,c]) gm[i,c] /
 *                      float(cnt[i,c]): the gradient of m[i,c] split EVENLY among all edges that attain the maximum */
int dc_sage_mean_fwd(const int32_t *ptr, const int32_t *other, const float *x, int64_t ldx, float *y, int64_t ldy,
                     int64_t N, int64_t F, dc_stream_t stream);
int dc_sage_mean_bwd(const int32_t *ptr_t, const int32_t *other_t, const int32_t *ptr, const float *gy, int64_t ldgy,
                     float *gx, int64_t ldgx, int64_t N, int64_t F, dc_stream_t stream);
int dc_sage_max_fwd(const int32_t *ptr, const int32_t *other, const float *x, int64_t ldx, float *m, int64_t ldm,
                    int32_t *cnt, int64_t ldc, int64_t N, int64_t F, dc_stream_t stream);
int dc_sage_max_bwd(const int32_t *ptr_t, const int32_t *other_t, const float *x, int64_t ldx, const float *m,
                    int64_t ldm, const int32_t *cnt, int64_t ldc, const float *gm, int64_t ldgm, float *gx,
                    int64_t ldgx, int64_t N, int64_t F, dc_stream_t stream);

/* ---- GINEConv: sum over a node's in-edges of relu(x_j + e_ji), the root term, and the backward (dc_gine.hip) ----
 * x fp32 [N, F] are the node rows, e fp32 [E, F] the edge rows in the order of the INPUT edges (row strides ld* >= F);
 * the key_row=1 set (ptr / other = source ids / perm = input edge id of every sorted position) and the key_row=0 set
 * (ptr_t / other_t = destination ids / perm_t) are those of an edge set taken as it is given - no self loop is added,
 * duplicates count, a row may have no edge - so perm is a bijection over the input edges.  eps: DEVICE pointer to one
 * float, read by the kernel (it may change between two replays of a captured launch); NULL: no root term.  Any F >= 1
 * (no width cap), any in-degree >= 0; 16-byte loads when F % 4 == 0 and every pointer and row stride is 16-byte
 * aligned.  Sums in a fixed order, no float atomics, no workspace, no host read: deterministic and capturable.  The
 * ReLU mask of the backward is recomputed from the same fp32 add as the forward (the same bits); relu'(0) = 0.
 * Arguments are checked before any HIP call, in the order of the SAGE entries: sizes, leading dimensions, then null
 * pointers, then aliasing.  N == 0 (dc_gine_bwd_e: E == 0) returns DC_OK before the null check.
 *   dc_gine_fwd   : s = 0; for p in [ptr[i], ptr[i+1]) in order s += max(x[other[p],c] + e[perm[p],c], 0);
 *                   y[i,c] = (1 + eps) * x[i,c] + s - 1 + eps formed first in fp32, then the product, then the add; plain
 *                   fp32 sums, no contraction.  e is never read for a set without edges.
 *   dc_gine_bwd_x : gx[j,c] = (1 + eps) * gy[j,c] + sum over the edges t out of j, in t order, of
 *                   (x[j,c] + e[perm_t[t],c] > 0) * gy[other_t[t],c]; the sum compensated
 *   dc_gine_bwd_e : ge[q,c] = (x[src[q],c] + e[q,c] > 0) * gy[dst[q],c] for every input edge q < E - src / dst: the two
 *                   rows of the int64 edge list the sets were built from; every row of ge is written exactly once; an
 *                   edge with an endpoint outside [0, N) gets a zero row */
int dc_gine_fwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const float *x, int64_t ldx,
                const float *e, int64_t lde, const float *eps, float *y, int64_t ldy, int64_t N, int64_t F,
                dc_stream_t stream);
int dc_gine_bwd_x(const int32_t *ptr_t, const int32_t *other_t, const int32_t *perm_t, const float *x, int64_t ldx,
                  const float *e, int64_t lde, const float *eps, const float *gy, int64_t ldgy, float *gx, int64_t ldgx,
                  int64_t N, int64_t F, dc_stream_t stream);
int dc_gine_bwd_e(const int64_t *src, const int64_t *dst, const float *x, int64_t ldx, const float *e, int64_t lde,
                  const float *gy, int64_t ldgy, float *ge, int64_t ldge, int64_t N, int64_t E, int64_t F,
                  dc_stream_t stream);

/* ---- Per-edge primitives of the "module per edge" layers (EdgeConv): pair rows and edge-row reductions (dc_edge.hip) ----
 * x fp32 [N, F] are the node rows; z [E, 2F], m [E, C] and their gradients are edge rows in the order of the INPUT edges
 * (row strides ld* >= the width).  src / dst: the two rows of the int64 edge list; the key_row=1 set (ptr / perm = input
 * edge id of every sorted position) and the key_row=0 set (ptr_t / perm_t) are those of that edge list taken as it is
 * given - no self loop is added, duplicates count, a row may have no edge.  Any width >= 1 (no cap), any in-degree >= 0;
 * 16-byte loads when the width % 4 == 0 and every pointer and row stride is 16-byte aligned.  Sums in a fixed order, no
 * float atomics, no workspace, no host read: deterministic and capturable.  Non-finite inputs as for the SAGE entries above
 * (contained sums, a NaN-propagating max that selects among +-Inf exactly).  Arguments
 * are checked before any HIP call, in the order of the GINE entries: sizes and leading dimensions, then null pointers,
 * then aliasing.  A zero row count (E for the entries that walk the input edges, N for the others) returns DC_OK
 * before the null check.  mode: 0 sum, 1 mean, 2 max.
 *   dc_edge_pair_fwd   : z[q,c] = x[dst[q],c]; z[q,F+c] = x[src[q],c] - x[dst[q],c] (one fp32 subtraction) for every
 *                        input edge q < E; every row of z is written exactly once; an edge with an endpoint outside
 *                        [0, N) gets a zero row of 2F
 *   dc_edge_pair_bwd   : gx[j,c] = the compensated sum of, first, gz[perm[p],c] - gz[perm[p],F+c] (the difference formed
 *                        first, in fp32) for p in [ptr[j], ptr[j+1]) in order, then gz[perm_t[t],F+c] for t in
 *                        [ptr_t[j], ptr_t[j+1]) in order; 0 for a node without edges
 *   dc_edge_reduce_fwd : sum: acc = 0, acc = acc + m[perm[p],c] in p order (plain fp32); mean: that sum / float(ptr[i+1]
 *                        - ptr[i]), a true division; max: y[i,c] = the maximum, cnt[i,c] (int32) = the number of edges
 *                        of the row that attain it - cnt is required for mode 2 and must be NULL otherwise; a row
 *                        without edges gives 0 (cnt 0)
 *   dc_edge_reduce_bwd : for every input edge q < E, i = dst[q]: sum gm[q,c] = gy[i,c]; mean gm[q,c] = gy[i,c] /
 *                        float(ptr[i+1] - ptr[i]); max gm[q,c] = (m[q,c] == y[i,c]) ? gy[i,c] / float(cnt[i,c]) : 0 - the
 *                        gradient of a maximum split EVENLY among all edges that attain it.  ptr is read in mode 1 only,
 *                        m / y / cnt in mode 2 only (NULL otherwise); every row of gm is written exactly once; an edge
 *                        with an endpoint outside [0, N) gets a zero row */
int dc_edge_pair_fwd(const int64_t *src, const int64_t *dst, const float *x, int64_t ldx, float *z, int64_t ldz,
                     int64_t N, int64_t E, int64_t F, dc_stream_t stream);
int dc_edge_pair_bwd(const int32_t *ptr, const int32_t *perm, const int32_t *ptr_t, const int32_t *perm_t,
                     const float *gz, int64_t ldgz, float *gx, int64_t ldgx, int64_t N, int64_t F, dc_stream_t stream);
int dc_edge_reduce_fwd(const int32_t *ptr, const int32_t *perm, const float *m, int64_t ldm, float *y, int64_t ldy,
                       int32_t *cnt, int64_t ldc, int mode, int64_t N, int64_t C, dc_stream_t stream);
int dc_edge_reduce_bwd(const int64_t *src, const int64_t *dst, const int32_t *ptr, const float *m, int64_t ldm,
                       const float *y, int64_t ldy, const int32_t *cnt, int64_t ldc, const float *gy, int64_t ldgy,
                       float *gm, int64_t ldgm, int mode, int64_t N, int64_t E, int64_t C, dc_stream_t stream);

/* ---- ChebConv: the scaled Laplacian's weights and one step of the Chebyshev recurrence (dc_cheb.hip) ----
 * The key_row=1 set (ptr / other = source ids) and the key_row=0 set (ptr_t / other_t = destination ids) are those of an
 * edge set taken as it is given (no self loop added, duplicates count).  A slot whose two ends coincide is a self loop:
 * it gets weight 0 and is not counted in a degree.  deg[j] = non-loop slots of the key_row=0 segment of j, the OUT-degree
 * (PyG get_laplacian scatters on edge_index[0]).  Fixed order, no float atomics, no host read: deterministic, capturable.
 * Arguments are checked before any HIP call: sizes, leading dimensions, then null pointers, then aliasing; N == 0 returns
 * DC_OK before the null check.
 *   dc_cheb_norm : mode 0 (sym): dinv[j] = 1 / sqrt(deg[j]), w = dinv[src] * dinv[dst]; mode 1 (rw): dinv[j] = 1 / deg[j],
 *                  w = dinv[src]; deg = 0 -> dinv = 0.  wl = (2 * -w) / lam in that order (one fp32 division), 0 for a
 *                  self loop; written per slot of the key_row=1 set (wl_fwd) and of the key_row=0 set (wl_bwd).  dinv
 *                  fp32 [N] is an output too (the workspace of the second launch).  lam > 0.  Two launches.
 *   dc_cheb_hop  : s = 0; for p in [ptr[i], ptr[i+1]) in order s += wl[p] * x[other[p],:] (product and sum rounded
 *                  separately); t = s + b * x[i,:]; y[i,:] = k * t + c * z[i,:] with k in {1, 2}, c in {-1, 0, +1} (c = 0:
 *                  z is not read, may be NULL, y = k * t); y2[i,:] = z2[i,:] - x[i,:] when y2 is not NULL.  x, z, y, z2,
 *                  y2: fp32 row-major views [N, F] with their own leading dimensions (column blocks of a slab).  y may
 *                  be z and y2 may be z2; neither may be x.  Any F >= 1; 16-byte accesses when F % 4 == 0 and every view
 *                  in use is 16-byte aligned with a row stride that is a multiple of 4.  One launch. */
int dc_cheb_norm(const int32_t *ptr, const int32_t *other, const int32_t *ptr_t, const int32_t *other_t, int mode,
                 float lam, float *dinv, float *wl_fwd, float *wl_bwd, int64_t N, dc_stream_t stream);
int dc_cheb_hop(const int32_t *ptr, const int32_t *other, const float *wl, const float *x, int64_t ldx, const float *z,
                int64_t ldz, float *y, int64_t ldy, const float *z2, int64_t ldz2, float *y2, int64_t ldy2, float b,
                int k, int c, int64_t N, int64_t F, dc_stream_t stream);

/* ---- GMMConv (MoNet): a mixture of K Gaussians over D pseudo-coordinates weights K column blocks (dc_gmm.hip) ----
 * h fp32 [N, K*M] (column k*M + c: kernel k, channel c), a fp32 [E, D] the pseudo-coordinates and w / gw fp32 [E, K]
 * (dense) in the order of the INPUT edges; mu / sigma fp32 [K, D] dense DEVICE arrays, read by the kernels (they may
 * change between two replays of a captured launch).  The key_row=1 set (ptr / other / perm) and the key_row=0 set
 * (ptr_t / other_t / perm_t) are those of an edge set of E edges taken as it is given, as for GINEConv.  Caps:
 * 1 <= K <= DC_GMM_MAX_K, 1 <= D <= DC_GMM_MAX_D, E * K < 2^31.  Any M >= 1, any in-degree; 16-byte accesses when
 * M % 4 == 0 and every pointer and row stride is 16-byte aligned.  Sums in a fixed order, no float atomics, no host
 * read: deterministic and capturable.  Arguments are checked before any HIP call: sizes, leading dimensions, then null
 * pointers, then aliasing.  N == 0 (dc_gmm_weights, dc_gmm_bwd_w, dc_gmm_bwd_params: E == 0) returns DC_OK before the
 * null check and launches nothing.  mean: 0 sums, 1 divides by the in-degree.
 *   dc_gmm_weights    : e = 0; for d in order e += (-0.5 * (t * t)) / (1e-15 + sigma[k,d]^2), t = a[q,d] - mu[k,d];
 *                       w[q,k] = exp(e) - float32 throughout, as torch evaluates PyG's expression
 *   dc_gmm_fwd        : s = 0; for p in [ptr[i], ptr[i+1]) in order, for k in order s += w[perm[p],k] * h[other[p],k*M+c]
 *                       (product and sum rounded separately); mean: s / float(deg) where deg > 0; + base[i,c] (base
 *                       NULL: none); relu: max(s, 0).  w is never read for a set without edges.
 *   dc_gmm_bwd_h      : gh[j,k*M+c] = sum over the edges t out of j, in t order, of w[perm_t[t],k] * gs[other_t[t],c];
 *                       gs[i,c] = gy[i,c] / float(deg_i) with deg from ptr, the key_row=1 pointer (mean), or gy[i,c]
 *                       (ptr NULL: add).  Every row of gh is written exactly once.
 *   dc_gmm_bwd_w      : gw[q,k] = sum_c gs[dst[q],c] * h[src[q],k*M+c] for every input edge q < E - src / dst: the two
 *                       rows of the int64 edge list the sets were built from; ptr as for dc_gmm_bwd_h; an edge with an
 *                       endpoint outside [0, N) gets a zero row
 *   dc_gmm_bwd_params : with t = gw[q,k] * w[q,k] and r = (a[q,d] - mu[k,d]) / (1e-15 + sigma[k,d]^2):
 *                       gmu[k,d] = sum_q t r, gsigma[k,d] = (sum_q t r r) * sigma[k,d] and, ga not NULL,
 *                       ga[q,d] = -sum_k t r.  Sums in double (as the dot products of dc_gmm_bwd_w): per chunk of edges into the 8-byte aligned workspace
 *                       (dc_gmm_params_workspace_bytes), then over the chunks in order.  Two launches, three with ga. */
#define DC_GMM_MAX_K 64
#define DC_GMM_MAX_D 16
int dc_gmm_weights(const float *a, int64_t lda, const float *mu, const float *sigma, float *w, int64_t E, int64_t K,
                   int64_t D, dc_stream_t stream);
int dc_gmm_fwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const float *w, const float *h,
               int64_t ldh, const float *base, int64_t ldb, int mean, int relu, float *y, int64_t ldy, int64_t N,
               int64_t E, int64_t K, int64_t M, dc_stream_t stream);
int dc_gmm_bwd_h(const int32_t *ptr_t, const int32_t *other_t, const int32_t *perm_t, const int32_t *ptr,
                 const float *w, const float *gy, int64_t ldgy, float *gh, int64_t ldgh, int64_t N, int64_t E,
                 int64_t K, int64_t M, dc_stream_t stream);
int dc_gmm_bwd_w(const int64_t *src, const int64_t *dst, const int32_t *ptr, const float *h, int64_t ldh,
                 const float *gy, int64_t ldgy, float *gw, int64_t N, int64_t E, int64_t K, int64_t M,
                 dc_stream_t stream);
int64_t dc_gmm_params_workspace_bytes(int64_t E, int64_t K, int64_t D);
int dc_gmm_bwd_params(const float *gw, const float *w, const float *a, int64_t lda, const float *mu,
                      const float *sigma, void *workspace, int64_t workspace_bytes, float *gmu, float *gsigma,
                      float *ga, int64_t ldga, int64_t E, int64_t K, int64_t D, dc_stream_t stream);

/* ---- SplineConv (SplineCNN): a B-spline over D pseudo-coordinates picks and weights S of K column blocks (dc_spline.hip) ----
 * h fp32 [N, K*M] (column k*M + c: weight matrix k, channel c), a fp32 [E, D] the pseudo-coordinates, b / gb fp32 [E, S]
 * and wi int32 [E, S] (dense) in the order of the INPUT edges, S = (degree+1)^D.  ks (int64 [D], the kernel size per
 * dimension) and open (int32 [D], non-zero: open spline) are HOST arrays: they and degree are copied into the kernel
 * arguments, K = prod ks[d].  The key_row=1 set (ptr / other / perm) and the key_row=0 set (ptr_t / other_t / perm_t) are
 * those of an edge set of E edges taken as it is given, as for GMMConv.  Caps: 1 <= D <= DC_SPLINE_MAX_D, 1 <= degree
 * <= 3, S <= DC_SPLINE_MAX_S, ks[d] >= 1, K <= DC_SPLINE_MAX_K, E * S < 2^31, N * K * M < 2^31.  Any M >= 1, any
 * in-degree; 16-byte accesses when M % 4 == 0 and every pointer and row stride is 16-byte aligned.  Sums in a fixed
 * order, no float atomics, no host read: deterministic and capturable.  Arguments are checked before any HIP call:
 * sizes, leading dimensions, then null pointers, then ks, then aliasing.  N == 0 (dc_spline_basis, dc_spline_bwd_b,
 * dc_spline_bwd_a: E == 0) returns DC_OK before the null check and launches nothing.  mean: 0 sums, 1 divides by the
 * in-degree.
 *   dc_spline_basis : for slot s, with k = s, wi = 0, off = 1, b = 1, for d in order: k_mod = k % (degree+1), k /= degree+1,
 *                     v = a[q,d] * float(ks[d] - degree*open[d]), wi += ((floor(v) + k_mod) mod ks[d]) * off, off *= ks[d],
 *                     b *= B_degree(v - floor(v), k_mod) - float32 throughout; the modulo is the non-negative one of
 *                     floor(v) clamped to +-2^30 (NaN: 0), so 0 <= wi < K for every a.
 *                     B_1(f,k) = 1 - f - k + 2fk; B_2 = (f^2/2 - f + 1/2, -f^2 + f + 1/2, f^2/2);
 *                     B_3 = ((1-f)^3, 3f^3 - 6f^2 + 4, -3f^3 + 3f^2 + 3f + 1, f^3) / 6
 *   dc_spline_fwd   : acc = 0; for p in [ptr[i], ptr[i+1]) in order: t = 0, for s in order t += b[perm[p],s] *
 *                     h[other[p], wi[perm[p],s]*M + c] (product and sum rounded separately), then acc += t (the edge's
 *                     message first, then the sum over the edges); mean: acc / float(deg) where deg > 0; + base[i,c]
 *                     (base NULL: none); relu: max(acc, 0).  b and wi are never read for a set without edges; wi must
 *                     hold values in [0, K) (those of dc_spline_basis).
 *   dc_spline_bwd_h : gh[j,k*M+c] = sum over the edges t out of j, in t order, and the slots s with wi[perm_t[t],s] == k,
 *                     in s order, of b[perm_t[t],s] * gs[other_t[t],c]; gs[i,c] = gy[i,c] / float(deg_i) with deg from
 *                     ptr, the key_row=1 pointer (mean), or gy[i,c] (ptr NULL: add).  Every column of every row of gh is
 *                     written exactly once, zeros included.
 *   dc_spline_bwd_b : gb[q,s] = sum_c gs[dst[q],c] * h[src[q], wi[q,s]*M + c] for every input edge q < E, formed in
 *                     double and rounded once - src / dst: the two rows of the int64 edge list the sets were built from;
 *                     ptr as for dc_spline_bwd_h; an edge with an endpoint outside [0, N) gets a zero row
 *   dc_spline_bwd_a : ga[q,d] = float(ks[d] - degree*open[d]) * sum_s gb[q,s] * B'(f_d, k_mod_d) * prod_{d' != d}
 *                     B(f_d', k_mod_d') with the float32 fractions f of dc_spline_basis, formed in double and rounded once */
#define DC_SPLINE_MAX_D 4
#define DC_SPLINE_MAX_S 64
#define DC_SPLINE_MAX_K 1024
int dc_spline_basis(const float *a, int64_t lda, DC_HOST const int64_t *ks, DC_HOST const int32_t *open,
                    int64_t degree, float *b, int32_t *wi, int64_t E, int64_t D, dc_stream_t stream);
int dc_spline_fwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const float *b, const int32_t *wi,
                  const float *h, int64_t ldh, const float *base, int64_t ldb, int mean, int relu, float *y,
                  int64_t ldy, int64_t N, int64_t E, int64_t S, int64_t K, int64_t M, dc_stream_t stream);
int dc_spline_bwd_h(const int32_t *ptr_t, const int32_t *other_t, const int32_t *perm_t, const int32_t *ptr,
                    const float *b, const int32_t *wi, const float *gy, int64_t ldgy, float *gh, int64_t ldgh,
                    int64_t N, int64_t E, int64_t S, int64_t K, int64_t M, dc_stream_t stream);
int dc_spline_bwd_b(const int64_t *src, const int64_t *dst, const int32_t *ptr, const int32_t *wi, const float *h,
                    int64_t ldh, const float *gy, int64_t ldgy, float *gb, int64_t N, int64_t E, int64_t S, int64_t K,
                    int64_t M, dc_stream_t stream);
int dc_spline_bwd_a(const float *gb, const float *a, int64_t lda, DC_HOST const int64_t *ks, DC_HOST const int32_t *open,
                    int64_t degree, float *ga, int64_t ldga, int64_t E, int64_t D, dc_stream_t stream);

/* ---- Point-set sampling and transfer (dc_pointops.hip; PyG fps, knn_interpolate) ----
 * Distances as in the neighbour search: d2 = ((dx*dx + dy*dy) + dz*dz) in fp32, each operation rounded on its own.
 * Fixed order, no float atomics, no host read: deterministic and capturable.  Positions select indices: behaviour
 * on non-finite input is unspecified here ("out of scope").  Arguments
 * are checked before any HIP call: sizes, leading dimensions, then null pointers, then aliasing.
 *   dc_fps : farthest point sampling of B graphs, one workgroup per graph.  x fp32 [N, >= 3] (leading dimension ldx).
 *            ptr int64 [B+1]: graph g owns the nodes [ptr[g], ptr[g+1]); optr int64 [B+1]: it writes the picks
 *            out[optr[g] .. optr[g+1]) (int64 global node ids, pick order).  ptr = optr = NULL: one graph of N nodes and
 *            M picks (B <= 1).  start int64 [B]: the first pick of every graph as a global node id (NULL, or a value
 *            outside the graph: its first node).  Then, dist = +inf and c = the start: for every further pick
 *            dist[j] = min(dist[j], d2(j, c)), c = the j with the largest dist[j], the lowest j among equals.  A graph
 *            without nodes or without picks is skipped, as is one whose offsets do not fit N and M.  max_n: at least
 *            the largest node count of a graph (a larger graph gets -1 picks).  max_n <= DC_FPS_RESIDENT_POINTS: points
 *            and distances stay in registers, no workspace.  Larger: dc_fps_workspace_bytes(N, max_n) = 16 N bytes,
 *            16-byte aligned, hold (x, y, z, dist) per node.  N == 0, B == 0, M == 0 or max_n == 0 returns DC_OK before
 *            the null check.  One launch.
 *   dc_knn_interpolate_fwd : x fp32 [Nx, F], pos_x [Nx, >= 3], pos_y [Ny, >= 3]; nbr int32 [Ny, k] and counts int32
 *            [Ny] as dc_neighbors_fill wrote them (rank order, -1 padding); 1 <= k <= DC_NEIGHBORS_MAX_CAP.  Per query
 *            i, over r < counts[i], j = nbr[i*k + r]: w = 1.0f / max(d2(pos_x[j], pos_y[i]), 1e-16f) (a true division);
 *            num[c] = num[c] + w * x[j,c] and den = den + w from 0 in rank order (product and sum rounded separately);
 *            y[i,c] = num[c] / den; a query without a neighbour gets a row of zeros.  w fp32 [Ny, k] (0 in the padding)
 *            and den fp32 [Ny] are written too when given (both or neither).  Any F >= 1; 16-byte accesses when F % 4
 *            == 0 and x, y and their row strides allow it.  Ny == 0 returns DC_OK before the null check.
 *   dc_knn_interpolate_bwd : ptr int64 [Nx+1], slots int64: slots[ptr[j] .. ptr[j+1]) are the positions s = i*k + r with
 *            nbr[s] == j, ascending.  gx[j,c] = the compensated sum, in that order, of w[s] * (gy[i,c] / den[i]); a
 *            source without a slot gets a zero row; every row of gx is written exactly once.  Nx == 0 returns DC_OK
 *            before the null check. */
#define DC_FPS_RESIDENT_POINTS 8192
int64_t dc_fps_resident_points(void);
int64_t dc_fps_workspace_bytes(int64_t N, int64_t max_n);
int dc_fps(const float *x, int64_t ldx, int64_t N, const int64_t *ptr, const int64_t *optr, int64_t B, int64_t max_n,
           const int64_t *start, int64_t *out, int64_t M, void *workspace, int64_t workspace_bytes, dc_stream_t stream);
int dc_knn_interpolate_fwd(const float *x, int64_t ldx, const float *pos_x, int64_t ldpx, const float *pos_y,
                           int64_t ldpy, const int32_t *nbr, const int32_t *counts, int k, float *y, int64_t ldy,
                           float *w, float *den, int64_t Nx, int64_t Ny, int64_t F, dc_stream_t stream);
int dc_knn_interpolate_bwd(const int64_t *ptr, const int64_t *slots, const float *w, const float *den, const float *gy,
                           int64_t ldgy, float *gx, int64_t ldgx, int k, int64_t Nx, int64_t Ny, int64_t F,
                           dc_stream_t stream);

/* ---- PointNetConv and global pooling (dc_pointnet.hip; PyG point_conv.py, global_*_pool) ----
 * The per-edge primitives of PointNet++ set abstraction on a BIPARTITE edge set - sources x_src [n_src, F] / pos_src
 * [n_src, >= 3], destinations pos_dst [n_dst, >= 3], src / dst the int64 rows of the edge list - and the per-graph
 * pooling.  The sorted sets are those of ONE adjacency over max(n_src, n_dst) rows (dc_graph_build): ptr / other / perm
 * by destination, ptr_t / other_t / perm_t by source.  loops != 0 (n_src == n_dst == N, the adjacency built with
 * self_loops): E + N edge rows, node i's loop at row E + i and LAST in its groups; an input edge with src == dst takes
 * no part.  Rules of dc_edge_*: fixed order, no float atomics, no host read, any width, 16-byte accesses where widths,
 * strides and pointers allow it.  Arguments are checked before any HIP call: sizes, leading dimensions, nulls, aliasing.
 *   dc_pointnet_pair_fwd   : z [E', F + 3]: z[q,:F] = x_src[src[q]] (a copy), z[q,F+d] = pos_src[src[q],d] -
 *            pos_dst[dst[q],d] (one fp32 subtraction); a loop row [x_src[i], +0, +0, +0].  src[q] outside [0, n_src) or
 *            dst[q] outside [0, n_dst): a zero row.  F == 0 is legal (x may be NULL).  zpad (0..3): that many further
 *            columns behind F + 3 are written as zeros (ldz >= F + 3 + zpad; the padding of a row stride rounded up to
 *            4 floats).  No row returns DC_OK.
 *   dc_pointnet_pair_bwd   : one lane group per node r < max(n_src, n_dst), compensated sums in the order of the sorted
 *            sets: gx[r,c] over gz[perm_t[t],c] (the loop row included), gpos_src[r,d] over gz[perm_t[t],F+d] and
 *            gpos_dst[r,d] = -(the sum over gz[perm[p],F+d]), both over input edges (id < E) alone; an edge whose other
 *            endpoint is outside its node set is left out.  Each of gx, gpos_src, gpos_dst may be NULL (skipped).
 *   dc_pointnet_reduce_bwd : the per-row gradient gm [E', C] of dc_edge_reduce_fwd over such a set (mode 0 sum, 1 mean,
 *            2 max with the even split among all rows that attain the maximum): i = dst[q], or q - E for a loop row;
 *            the mean divides by ptr[i+1] - ptr[i] (the loop counts).  A zero row for dst[q] outside [0, n_dst), src[q]
 *            outside [0, n_all) (n_all >= n_dst: the rows of the adjacency) and, with loops, src[q] == dst[q].
 *   dc_pool_fwd : y [B, C] = sum (mode 0) / mean (1) / max (2, cnt int32 [B, C] = the rows that attain it) of the rows
 *            [ptr[g], ptr[g+1]) of x [N, C] (ptr int64 [B+1]; NULL: one graph [0, N), B == 1).  One workgroup per
 *            (graph, block of 16 (64 with 16-byte access) columns): 16 slots of 16 lanes, slot s takes the rows a + s,
 *            a + s + 16, ... in ascending order from 0 (-inf), the 16 partial results are merged in slot order.  A graph
 *            without rows gets 0 (cnt 0).  B == 0 returns DC_OK.
 *   dc_pool_bwd : gx [N, C]: g = batch[r] (NULL with ptr NULL: one graph): gy[g] (sum), gy[g] / float(rows of g) (mean),
 *            (x[r,c] == y[g,c]) ? gy[g,c] / float(cnt[g,c]) : 0 (max); g outside [0, B): a zero row.  N == 0: DC_OK. */
int dc_pointnet_pair_fwd(const int64_t *src, const int64_t *dst, const float *x, int64_t ldx, const float *pos_src,
                         int64_t ldps, const float *pos_dst, int64_t ldpd, float *z, int64_t ldz, int64_t n_src,
                         int64_t n_dst, int64_t E, int64_t F, int loops, int zpad, dc_stream_t stream);
int dc_pointnet_pair_bwd(const int32_t *ptr, const int32_t *other, const int32_t *perm, const int32_t *ptr_t,
                         const int32_t *other_t, const int32_t *perm_t, const float *gz, int64_t ldgz, float *gx,
                         int64_t ldgx, float *gpos_src, int64_t ldgps, float *gpos_dst, int64_t ldgpd, int64_t n_src,
                         int64_t n_dst, int64_t E, int64_t F, int loops, dc_stream_t stream);
int dc_pointnet_reduce_bwd(const int64_t *src, const int64_t *dst, const int32_t *ptr, const float *m, int64_t ldm,
                           const float *y, int64_t ldy, const int32_t *cnt, int64_t ldc, const float *gy, int64_t ldgy,
                           float *gm, int64_t ldgm, int mode, int64_t n_all, int64_t n_dst, int64_t E, int64_t C,
                           int loops, dc_stream_t stream);
int dc_pool_fwd(const int64_t *ptr, const float *x, int64_t ldx, float *y, int64_t ldy, int32_t *cnt, int64_t ldc,
                int mode, int64_t N, int64_t B, int64_t C, dc_stream_t stream);
int dc_pool_bwd(const int64_t *batch, const int64_t *ptr, const float *x, int64_t ldx, const float *y, int64_t ldy,
                const int32_t *cnt, int64_t ldc, const float *gy, int64_t ldgy, float *gx, int64_t ldgx, int mode,
                int64_t N, int64_t B, int64_t C, dc_stream_t stream);

/* ---- packing helpers of the narrow-layer path (F_in = 21 / 25) ----------------
 * A TAGConv layer whose K+1 column blocks are narrow runs its dense block over ONE K segment:
 * the hop slab [N, wpad] (wpad = (K+1)*F rounded up to 16).  pack_input: slab[:, 0:F] = x and
 * slab[:, width:wpad] = 0.  pack_weights: wcat[Fo, wpad] = [ws[0] | ... | ws[nw-1] | 0]. */
int dc_tag_pack_input(const float *x, int64_t ldx, float *slab, int64_t ld_slab, int64_t N,
                      int64_t F, int64_t width, int64_t wpad, dc_stream_t stream);
int dc_tag_pack_weights(const float *const *ws, int nw, float *wcat, int64_t Fo, int64_t fi,
                        int64_t wpad, dc_stream_t stream);

/* ---- row kernels of the blocked cross-attention -------------------
 * models/model.py:7-21: per head  softmax(head(x_soft) . head(x_rigid)^T, dim=-1) . x_rigid, unmasked,
 * no 1/sqrt(d).  The score matrix exists only for a block of soft rows s [rows, ld]; its three
 * GEMMs run on the h2 dense entries above and these kernels do the row-wise parts in place:
 *   softmax_rows: s[i,0:n] <- softmax(s[i,0:n]), s[i,n:npad] <- 0, lse[i] = log sum_j exp(s[i,j])
 *   exp_rows    : s[i,0:n] <- exp(s[i,0:n] - lse[i]), s[i,n:npad] <- 0   (backward recompute)
 *   ds_rows     : dp[i,j] <- p[i,j] * (dp[i,j] - delta[i]) for j < npad; rowmax[i] = max_j |.| */
/* Flash-style FORWARD of one attention head (models/model.py:13-21), d = dv = DC_ATTN_FLASH_D:
 *   o[i,:] = sum_j softmax_j(q[i,:] . k[j,:]) v[j,:],   lse[i] = log sum_j exp(q[i,:] . k[j,:]),  j < nr
 * in ONE launch - the scores of a 128-query tile never leave the compute unit (online softmax over 32-key tiles).
 * Operands as the blocked form hands them to dc_tag_linear_fwd_h2p: q fp32 [ns, ldq] with its row maxima
 * (dc_rowabsmax_f32); k_image = dc_tag_weight_prep of the keys [nr_padded, d], k_unscale from dc_attn_flash_prep;
 * vt_image / vt_rowmax = the transposed image of the values (V^T [dv, nr_padded]) AFTER dc_attn_flash_prep; nr_padded % 32 == 0,
 * rows nr..nr_padded of k / v are zero padding and are masked.  Same products, same order as the blocked form: score (i, j) is bit-identical to
 * dc_tag_linear_fwd_h2p's, so the blocked backward (dc_tag_linear_fwd_h2p_exp with this lse) recomputes exactly
 * the weights that were normalised here. */
#define DC_ATTN_FLASH_D 256
/* Operand preparation of dc_attn_flash_fwd, two small launches: (i) rewrites the transposed image of
 * dc_tag_weight_prep vt_image [dv, nr_padded] IN PLACE into the key order the kernel consumes (the four 4-key chunks of
 * every plane of every 16-key record in the order 0, 2, 1, 3: a lane of the transposed score tile holds the weights
 * of keys {4h..4h+3, 8+4h..11+4h}; the rewrite is its own inverse); (ii) k_unscale[j] = the exact power of two that
 * undoes the scaling of row j of the key image (from k_rowmax of dc_tag_weight_prep), which the kernel fetches with
 * scalar loads. */
int dc_attn_flash_prep(void *vt_image, int64_t dv, int64_t nr_padded, const float *k_rowmax, float *k_unscale,
                       dc_stream_t stream);
int dc_attn_flash_fwd(const float *q, int64_t ldq, const float *q_rowmax, const void *k_image,
                      const float *k_unscale, const void *vt_image, const float *vt_rowmax, int64_t ns,
                      int64_t nr, int64_t nr_padded, int64_t d, float *o, int64_t ldo, float *lse,
                      dc_stream_t stream);
/* The backward's score-sized operands for ALL query rows in one launch (replaces, per 2,048-row block, dc_tag_linear_fwd_h2p_exp
 * + dc_tag_linear_fwd_h2p + dc_attn_ds_rows):  p_out[i, j] = exp(q_i . k_j - lse[i]),  ds_out[i, j] = p_ij (dp_ij - delta_i)
 * with dp_ij = go_i . v_j and delta_i = sum_j p_ij dp_ij / sum_j p_ij formed from the SAME recomputed p and dp (two
 * sweeps over the keys per 128-query tile; nothing score-sized is read back), ds_rowmax[i] = max_j |ds_ij|; columns
 * nr..nr_padded come out as exact zeros.  q / go fp32 with their row maxima; k_image / v_image = dc_tag_weight_prep images
 * of the keys' and the values' ROWS [nr_padded, d], k_unscale / v_unscale from dc_attn_flash_prep (dv = 0 skips the
 * image rewrite); d = dv = DC_ATTN_FLASH_D, nr_padded % 32 == 0, p_out / ds_out [ns, ldp >= nr_padded].  Products as in
 * the blocked form (scores bit-identical to dc_tag_linear_fwd_h2p's).
 * SINGLE-SWEEP mode (delta_in / eps_out not NULL, both [ns]): ds_out = p (dp - delta_in) with the caller's delta
 * (rowsum(dO o O)) and eps_out[i] = sum_j ds_ij / sum_j p_ij, i.e. consistent delta = delta_in + eps: half the matrix
 * work; consumers whose result is sensitive to sum_j ds_ij != 0 take ds - eps_i p (dc_tag_linear_bwd_dw_h2_corr). */
int dc_attn_flash_ds(const float *q, int64_t ldq, const float *q_rowmax, const float *go, int64_t ldgo,
                     const float *go_rowmax, const void *k_image, const float *k_unscale, const void *v_image,
                     const float *v_unscale, const float *lse, int64_t ns, int64_t nr, int64_t nr_padded, int64_t d,
                     float *p_out, float *ds_out, int64_t ldp, float *ds_rowmax, const float *delta_in,
                     float *eps_out, dc_stream_t stream);
int dc_attn_softmax_rows(float *s, int64_t ld, int64_t rows, int64_t n, int64_t npad, float *lse,
                         dc_stream_t stream);
int dc_attn_exp_rows(float *s, int64_t ld, int64_t rows, int64_t n, int64_t npad, const float *lse,
                     dc_stream_t stream);
int dc_attn_ds_rows(const float *p, float *dp, int64_t ld, int64_t rows, int64_t npad,
                    const float *delta, float *rowmax, dc_stream_t stream);

/* ---- optimizer step of the path's training loop -----------------------------
 * torch.optim.Adam(lr) at its defaults (train.py:20: no weight decay, no amsgrad) over ONE
 * flat fp32 bucket of parameters / gradients / moments: a single elementwise pass.  `step` is a
 * zero-initialised device buffer of DC_ADAM_STEP_WORDS 32-bit words: step[0] (float) counts the
 * completed updates and is advanced on the device by the launch itself (the other words are its
 * internal tickets), so the call is replayable inside a hipGraph.  zero_grad != 0 also clears g (optimizer.zero_grad(), train.py:71). */
#define DC_ADAM_STEP_WORDS 34
int dc_adam_flat(float *p, float *g, float *m, float *v, int64_t n, float *step, float lr,
                 float beta1, float beta2, float eps, int zero_grad, dc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DEFORMCONTACT_H */
