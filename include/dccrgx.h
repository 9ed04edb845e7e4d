/*
 * dccrgx — C ABI of the MI355X-native dccrg neighbor-stencil + halo path.
 *
 * One opaque grid per process (one process per GPU).  Cell payloads live in
 * HBM as structure-of-arrays "fields"; every field is indexed by a *slot*:
 *
 *     [0, n_inner)              local cells without remote neighbors
 *     [n_inner, n_local)        local cells with remote neighbors
 *                               (both runs in ascending id on unrefined grids,
 *                               in Morton order of the cells' min corners when
 *                               max refinement level > 0, for locality)
 *     [n_local, n_local+n_recv) copies of remote neighbors, grouped by owner
 *                               (ascending rank), ascending id inside a group
 *                               = the halo exchange wire order
 *     [.., n_slots)             remote cells that only have local cells as
 *                               neighbors_to (no payload is ever received)
 *
 * State per rank is the rank's own leaves plus the "ghost" leaves around
 * them (within max(neighborhood length, 1) level-0 cells), never the whole
 * grid: the reference's global cell_process map (dccrg.hpp:7197) has no
 * counterpart.
 *
 * Every entry point returns 0 on success and a negative code on failure;
 * dccrgx_last_error() then describes the failure.  Every function cites the
 * reference interface (lkotipal/dccrg @ 2024-10-24, dccrg.hpp unless noted)
 * it replaces.
 */
#ifndef DCCRGX_H
#define DCCRGX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dccrgx_grid dccrgx_grid;

#define DCCRGX_ABI_VERSION 10 /* dccrgx_abi_version() of a matching library */

#define DCCRGX_OK 0
#define DCCRGX_EINVAL -1   /* bad argument / wrong state  (std::invalid_argument) */
#define DCCRGX_EHIP -2     /* HIP runtime failure */
#define DCCRGX_ECOMM -3    /* RCCL failure */
#define DCCRGX_ERANGE -4   /* caller buffer too small; *n holds the needed size */
#define DCCRGX_ENOTFOUND -5 /* unknown cell (reference returns nullptr) */

/* cell selections for dccrgx_get_cells (iterator ranges dccrg.hpp:7478-7602) */
#define DCCRGX_CELLS_LOCAL 0   /* local_cells()  */
#define DCCRGX_CELLS_INNER 1   /* inner_cells()  */
#define DCCRGX_CELLS_OUTER 2   /* outer_cells()  */
#define DCCRGX_CELLS_REMOTE 3  /* remote_cells() = remote_cells_on_process_boundary */
#define DCCRGX_CELLS_ALL 4     /* all_cells()    */

/* sweep regions */
#define DCCRGX_REGION_ALL 0
#define DCCRGX_REGION_INNER 1
#define DCCRGX_REGION_OUTER 2

const char* dccrgx_last_error(void);
int dccrgx_abi_version(void);

/* ---- communicator / lifetime ---------------------------------------------
 * dccrgx_get_unique_id: rank 0 creates the 128-byte RCCL bootstrap id that the
 * caller broadcasts (replaces Dccrg::initialize(MPI_Comm) 472-552's
 * MPI_Comm_dup, 7622-7687).  nccl_id may be NULL when size == 1. */
int dccrgx_get_unique_id(void* out_128_bytes);
int dccrgx_create(int rank, int size, int device, const void* nccl_id, dccrgx_grid** out);
int dccrgx_destroy(dccrgx_grid* g);

/* A host transport instead of RCCL (ranks sharing one GPU, MPI programs,
 * tests): one grouped point-to-point exchange with every rank - send
 * send_bytes[p] bytes from send[p] to rank p and receive recv_bytes[p] bytes
 * from rank p into recv[p] (entries of 0 bytes and the own rank post
 * nothing; all buffers are host memory).  Every rank calls it the same number
 * of times in the same order, as MPI point-to-point calls in the reference
 * (start_user_data_transfers 10564-10997).  Returns 0 on success.  The
 * library builds its collectives (All_Gather, Allreduce) and the halo and
 * migration payload transfers on it. */
typedef int (*dccrgx_exchange_fn)(void* ctx, const void* const* send, const size_t* send_bytes, void* const* recv,
                                  const size_t* recv_bytes);
int dccrgx_create_with_exchange(int rank, int size, int device, dccrgx_exchange_fn fn, void* ctx, dccrgx_grid** out);
/* number of visible GPUs (for choosing a device per rank) */
int dccrgx_device_count(int* n);

/* ---- setup, before initialize (dccrg.hpp:8120-8230) ---------------------- */
int dccrgx_set_initial_length(dccrgx_grid* g, const uint64_t length[3]);   /* 8120 */
int dccrgx_set_maximum_refinement_level(dccrgx_grid* g, int level);        /* 8154 */
int dccrgx_set_periodic(dccrgx_grid* g, int x, int y, int z);              /* 8183 */
int dccrgx_set_neighborhood_length(dccrgx_grid* g, unsigned length);       /* 8206 */
int dccrgx_get_maximum_refinement_level(dccrgx_grid* g, int* level);
/* the setup as the library holds it, e.g. after load_grid_data read it from
 * a file: length in level-0 cells, periodicity (ABI 8) */
int dccrgx_get_initial_length(dccrgx_grid* g, uint64_t length[3]);
int dccrgx_get_periodic(dccrgx_grid* g, int periodic[3]);
/* get_neighborhood_length (6725): the length set, or read from a grid file
 * by load_grid_data (ABI 8) */
int dccrgx_get_neighborhood_length(dccrgx_grid* g, unsigned* length);
/* initialize(): level-0 cells, block partition (create_level_0_cells
 * 7967-8102), device neighbor build (initialize_neighbors 8240-8289 and
 * update_remote_neighbor_info / send-receive lists 8590-9309).  472 */
int dccrgx_initialize(dccrgx_grid* g);
/* Cartesian_Geometry::set (dccrg_cartesian_geometry.hpp:184) */
int dccrgx_set_geometry(dccrgx_grid* g, const double start[3], const double level_0_cell_length[3]);

/* Cartesian_Geometry::get_center / get_length (dccrg_cartesian_geometry.hpp:
 * 282-362) of n cells: 3 doubles per cell each (either output may be NULL);
 * NaN for invalid ids */
/* Cartesian_Geometry::get_start / get_level_0_cell_length (ABI 8); either
 * output may be NULL */
int dccrgx_get_geometry(dccrgx_grid* g, double start[3], double level_0_cell_length[3]);
/* The grid file's geometry block of a Stretched_Cartesian_Geometry
 * (Stretched_Cartesian_Geometry::write / read,
 * dccrg_stretched_cartesian_geometry.hpp:652-800: int id 2, 3 x uint64
 * coordinate counts, the coordinates as doubles), which save_grid_data then
 * writes instead of the Cartesian block (n = 0: the Cartesian block again);
 * DCCRGX_EINVAL for other bytes.  After load_grid_data of a file with such a
 * block, dccrgx_get_geometry_block returns it (*n = 0 for a Cartesian file;
 * out = NULL: the size only) and the library's own geometry takes each
 * dimension's start and first cell length (ABI 10). */
int dccrgx_set_geometry_block(dccrgx_grid* g, const void* bytes, size_t n);
int dccrgx_get_geometry_block(dccrgx_grid* g, void* out, size_t cap, size_t* n);
int dccrgx_geometry_batch(dccrgx_grid* g, const uint64_t* ids, size_t n, double* center, double* length);
/* Stretched_Cartesian_Geometry as the library's own geometry: per dimension
 * the level-0 cell boundaries, n[d] == length[d] + 1 (set_initial_length
 * comes first) finite, strictly increasing values (set 172-210; DCCRGX_EINVAL
 * otherwise, dccrgx_last_error names the dimension, nothing changes); before
 * or after initialize.  From then on dccrgx_geometry_batch,
 * dccrgx_geometry_fill, dccrgx_get_existing_cells_at and dccrgx_particles_step
 * answer with its get_center / get_length (298-403) and get_real_coordinate /
 * get_indices (504-607; a coordinate at a dimension's first boundary belongs
 * to the first cell), the geometry block is the one its write() makes of the
 * coordinates, and the advection sweeps read the length fields.  The built-in
 * solvers follow it too: dccrgx_poisson_cache computes its factors from the
 * get_length of every cell and of every kept face neighbor,
 * dccrgx_advection_initialize takes center and length from it, and
 * dccrgx_advection_adapt's reset pass writes its velocities, lengths and the
 * next time step's bound from it (dccrgx_advection_length_source stays 0).
 * A grid that holds a file block only (dccrgx_set_geometry_block,
 * load_grid_data) has no coordinates: those three calls then see each
 * dimension's start and first cell length, as before.
 * dccrgx_set_geometry returns the grid to Cartesian; dccrgx_set_geometry_block
 * and load_grid_data leave a file block only, without coordinates.  The
 * finest cells must be wider than the spacing of doubles at their level-0
 * cell's ends (checked at first device use).
 * dccrgx_get_stretched_geometry: dimension dim's coordinates (*n = 0 when no
 * stretched geometry is active; out = NULL: the count only). */
int dccrgx_set_stretched_geometry(dccrgx_grid* g, const double* const coords[3], const size_t n[3]);
int dccrgx_get_stretched_geometry(dccrgx_grid* g, int dim, double* out, size_t cap, size_t* n);
/* The fp64 center and / or length of every slot's cell (local cells and
 * remote copies) written into fixed-size fp64 fields on the device; either
 * array may be NULL, an entry -1 skips that component.  Cartesian: the
 * expressions of dccrgx_advection_initialize, so the lengths are bitwise the
 * ones it writes.  Stretched: those of dccrgx_geometry_batch.  A field whose
 * device pointer was handed out is refused. */
int dccrgx_geometry_fill(dccrgx_grid* g, const int center_fields[3], const int length_fields[3]);

/* ---- mapping (dccrg_mapping.hpp) — host-side scalar queries -------------- */
uint64_t dccrgx_get_cell_from_indices(dccrgx_grid* g, const uint64_t indices[3], int level); /* 153 */
int dccrgx_get_indices(dccrgx_grid* g, uint64_t cell, uint64_t indices[3]);                 /* 217 */
int dccrgx_get_refinement_level(dccrgx_grid* g, uint64_t cell);                             /* 261 */
uint64_t dccrgx_get_last_cell(dccrgx_grid* g);                                              /* 651 */
/* The same id math as the device kernels evaluate it, for n ids (valid
 * before initialize): level[i] (-1 for an invalid id) and 15 words per id in
 * out, following dccrg_mapping.hpp: indices x,y,z (get_indices 217), length
 * in indices (297), parent (get_parent 367), first child (get_child 338),
 * level-0 parent (479), siblings x8 (get_siblings 449); error_cell (0) in
 * every word of an invalid id. */
int dccrgx_mapping_batch(dccrgx_grid* g, const uint64_t* ids, size_t n, int32_t* level, uint64_t* out);

/* ---- queries ------------------------------------------------------------- */
/* get_cells(criteria={}, sorted=true) restricted to a selection; 651 */
int dccrgx_get_cells(dccrgx_grid* g, int which, uint64_t* out, size_t cap, size_t* n);
int dccrgx_get_counts(dccrgx_grid* g, size_t* n_inner, size_t* n_outer, size_t* n_recv, size_t* n_slots);
/* get_neighbors_of 819 (stencil order, error cells dropped as in 4634);
 * offsets as int32 x,y,z triples.  Returns DCCRGX_ENOTFOUND for non-local cells. */
int dccrgx_get_neighbors_of(dccrgx_grid* g, uint64_t cell, uint64_t* ids, int32_t* offsets, size_t cap, size_t* n);
/* all slot ids (slot order, see the layout above) */
int dccrgx_get_slot_ids(dccrgx_grid* g, uint64_t* out, size_t cap, size_t* n);
/* bulk download of a local CSR in slot order (rows = local slots):
 * kind 0 neighbors_of (aux = x,y,z offsets), 1 neighbors_to, 2 face
 * neighbors (aux = direction), 3 iterator cell.neighbors_of (update_cell_
 * pointers 11451-11500: only-of then both, each in (id, offset) order; aux
 * = x,y,z offsets).
 * ptr has n_local + 1 entries; *n = number of entries. */
int dccrgx_download_csr(dccrgx_grid* g, int kind, uint32_t* ptr, uint64_t* ids, int32_t* aux, size_t cap, size_t* n);
/* get_cells(criteria, exact_match, neighborhood_id, sorted=true) 651 with
 * is_neighbor_type_match 2946-3053: local cells whose neighbor types (the
 * bits has_local_neighbor_of 1, _to 2, has_remote_neighbor_of 4, _to 8 of
 * dccrg.hpp:95-142, from neighbors_of / neighbors_to of the neighborhood)
 * intersect the OR of the criteria (exact_match = 0) or equal one of them
 * (exact_match = 1); nc = 0 returns every local cell; ascending id */
int dccrgx_get_cells_by_criteria(dccrgx_grid* g, const int32_t* criteria, size_t nc, int exact_match, int hood_id,
                                 uint64_t* out, size_t cap, size_t* n);
/* slots of many cells (-1 when a cell has no slot on this rank) */
int dccrgx_get_slots(dccrgx_grid* g, const uint64_t* ids, size_t n, int64_t* slots);
/* bulk download of a user neighborhood's CSR in slot order (kind 0
 * neighbors_of with x,y,z offsets, 1 neighbors_to); as dccrgx_download_csr */
int dccrgx_download_user_csr(dccrgx_grid* g, int hood_id, int kind, uint32_t* ptr, uint64_t* ids, int32_t* offsets,
                             size_t cap, size_t* n);
/* get_neighbors_to 883 (ascending id, offsets 0) */
int dccrgx_get_neighbors_to(dccrgx_grid* g, uint64_t cell, uint64_t* ids, size_t cap, size_t* n);
/* get_face_neighbors_of 2806 (dirs -1,+1,-2,+2,-3,+3): a local cell from the
 * device face lists; a remote cell this process knows (e.g. a copy in
 * all_cells()) from its known leaves, DCCRGX_ENOTFOUND if one of its faces
 * lies beyond the ghost region */
int dccrgx_get_face_neighbors_of(dccrgx_grid* g, uint64_t cell, uint64_t* ids, int32_t* dirs, size_t cap, size_t* n);
/* is_local 3270, get_process 5807 (-1 for unknown cells) */
int dccrgx_is_local(dccrgx_grid* g, uint64_t cell);
int dccrgx_get_process(dccrgx_grid* g, uint64_t cell);
/* slot of a local cell or remote copy (-1 if none) */
int64_t dccrgx_get_slot(dccrgx_grid* g, uint64_t cell);
/* peers of this rank and their send/receive lists (cells_to_send /
 * cells_to_receive 6900-6914, 8590-8752; ascending id = wire order) */
int dccrgx_get_peers(dccrgx_grid* g, int32_t* peers, size_t cap, size_t* n);
int dccrgx_get_cells_to_send(dccrgx_grid* g, int peer, uint64_t* ids, size_t cap, size_t* n);
int dccrgx_get_cells_to_receive(dccrgx_grid* g, int peer, uint64_t* ids, size_t cap, size_t* n);
/* the leaves this rank knows with their processes, ascending id: its own
 * and its ghost leaves (the reference's get_cell_process 6848 returns every
 * leaf of the grid); ids == NULL: *n = count only */
int dccrgx_get_cell_process(dccrgx_grid* g, uint64_t* ids, int32_t* owners, size_t cap, size_t* n);

/* find_neighbors_of(cell, neighborhood) 4339-4680 for any list of n_items
 * offsets (3 x int32 each, cell-sized units): the (id, x/y/z offset) pairs in
 * item order, a finer box as its 8 cells in z-order, error cells dropped -
 * the sequence the reference's walk over the face cache produces.
 * DCCRGX_ENOTFOUND for a cell this process does not know (the reference
 * throws, 4354-4362).  For a local cell every item's box must lie within the
 * process's ghost region (max(neighborhood length, 1) level-0 cells around
 * the cell's level-0 parent; DCCRGX_EINVAL otherwise); for a remote cell the
 * list may be incomplete, as the reference documents (4327-4328). */
int dccrgx_find_neighbors_of(dccrgx_grid* g, uint64_t cell, const int32_t* items, size_t n_items, uint64_t* ids,
                             int32_t* offsets, size_t cap, size_t* n);
/* get_neighbors_ 7098-7109 (the face-neighbor cache of update_neighbors_
 * 9313-9458): per leaf the cell at the min corner just across each face,
 * directions -x,+x,-y,+y,-z,+z, error_cell (0) where none.  The reference
 * holds an entry for every leaf of the grid; here every known leaf whose six
 * probes land in level-0 cells this process knows (all own leaves and the
 * inner ghosts): n leaves ascending in ids, 6 x n entries in nbrs.  Costs
 * O(known leaves) on the host (a query for tests, not a sweep). */
int dccrgx_get_face_cache(dccrgx_grid* g, uint64_t* ids, uint64_t* nbrs, size_t cap, size_t* n);
/* unpin_all_cells 6017: drop every pin of this process (collective in the
 * reference; pins here are held by the process owning the cell) */
int dccrgx_unpin_all_cells(dccrgx_grid* g);

/* get_number_of_update_send_cells / _receive_cells 5382-5490 */
int dccrgx_get_number_of_update_cells(dccrgx_grid* g, uint64_t* n_send, uint64_t* n_receive);

/* ---- refinement (refine_completely 2434, unrefine_completely 2560,
 * dont_unrefine 2679, dont_refine 2744, stop_refining 3461 -> override_refines
 * 9991, induce_refines 9591, override_unrefines 9796, execute_refines 10104).
 * Requests are local leaves only (ENOTFOUND otherwise; unrefine_completely
 * also when a sibling has children).  stop_refining is collective: refined
 * leaves get their 8 children (owner and, here, payload inherited), merged
 * families become their parent (owner of the first child, payload zeroed);
 * the removed children's payloads move to the parent's process, where
 * get_removed_cells / dccrgx_removed_field_* expose them until the next
 * stop_refining or balance_load (unrefined_cell_data 7250, 3497). */
int dccrgx_refine_completely(dccrgx_grid* g, uint64_t cell);
int dccrgx_unrefine_completely(dccrgx_grid* g, uint64_t cell);
int dccrgx_dont_unrefine(dccrgx_grid* g, uint64_t cell);
int dccrgx_dont_refine(dccrgx_grid* g, uint64_t cell);
int dccrgx_stop_refining(dccrgx_grid* g, uint64_t* new_cells, size_t cap, size_t* n);
/* removed cells whose parent is local, in the order of the payload arrays
 * below (the kept children ascending, then per source rank ascending) */
int dccrgx_get_removed_cells(dccrgx_grid* g, uint64_t* ids, size_t cap, size_t* n);
/* a field's payloads of those cells: n x elem_bytes */
int dccrgx_removed_field_download(dccrgx_grid* g, int field_id, void* host, size_t cap_bytes);
int dccrgx_removed_field_device_ptr(dccrgx_grid* g, int field_id, void** ptr);
/* the local cells created by the last stop_refining (ascending) */
int dccrgx_get_new_cells(dccrgx_grid* g, uint64_t* new_cells, size_t cap, size_t* n);

/* Replace the whole leaf set and its partition (every rank passes the same
 * global list: ids strictly ascending, owners in [0, size)); the rank keeps
 * its own and its ghost leaves.  Setup path for a mesh + partition handed
 * over from outside (as load_grid_data 1089-2425 reads every cell's record);
 * payloads of cells that stay local are kept.  No communication. */
int dccrgx_set_cells(dccrgx_grid* g, const uint64_t* ids, const int32_t* owners, size_t n);

/* ---- user neighborhoods (add_neighborhood 6383-6520, remove_neighborhood
 * 6530-6570, get_neighbors_of/_to(cell, id) 819/883, the id's
 * cells_to_send / _receive, update_copies_of_remote_neighbors(id) 966).
 * Offsets: 3 x int32 per item, within the default neighborhood (face
 * offsets when its length is 0), never (0,0,0); a rejected set returns
 * DCCRGX_EINVAL where the reference returns false.  Identical calls on every
 * rank.  kind 0 = neighbors_of (offsets filled), 1 = neighbors_to. */
#define DCCRGX_DEFAULT_HOOD -0xDCC  /* default_neighborhood_id (dccrg.hpp:93) */
int dccrgx_add_neighborhood(dccrgx_grid* g, int id, const int32_t* offsets, size_t n);
int dccrgx_remove_neighborhood(dccrgx_grid* g, int id);
int dccrgx_get_user_neighbors(dccrgx_grid* g, int id, uint64_t cell, int kind, uint64_t* ids, int32_t* offsets,
                              size_t cap, size_t* n);
int dccrgx_get_user_update_list(dccrgx_grid* g, int id, int peer, int receive, uint64_t* ids, size_t cap, size_t* n);
int dccrgx_update_copies_of_remote_neighbors_hood(dccrgx_grid* g, int id);

/* ---- grid files (save_grid_data 1089-1740, load_grid_data 1742-2425;
 * layout 1104-1120).  save: every rank calls it with the same arguments;
 * rank 0 writes the header bytes at `offset`, every rank its cells' records
 * and data: per cell the payloads of the transferred fields in field order,
 * a fixed-size field's window (dccrgx_set_field_window; what the cell's
 * get_mpi_datatype describes) and a variable-size field's bytes of the cell.
 * load: on a created, not yet initialized grid whose transferred fields are
 * registered as at save time; initializes the grid from the file (length,
 * refinement level, neighborhood length, periodicity, geometry), creates the
 * file's cells with the level-0 block partition inherited by children, and
 * reads the local cells' payloads; a variable-size field (at most one) takes
 * the rest of each record after the fixed-size fields that follow it. */
int dccrgx_save_grid_data(dccrgx_grid* g, const char* path, uint64_t offset, const void* header, size_t header_bytes);
int dccrgx_load_grid_data(dccrgx_grid* g, const char* path, uint64_t offset, size_t header_bytes);
/* the split load (start_loading_grid_data 1795, continue_loading_grid_data
 * 2112, finish_loading_grid_data 2380), for records whose layout the caller
 * learns from their first bytes (tests/restart/variable_cell_data.cpp):
 * start initializes the grid and its cells as load does and reads no
 * payload; each continue reads the next bytes of every local cell's record
 * into one field and advances the cell's position past them - a fixed-size
 * field its window (sizes NULL), a variable-size field sizes[s] bytes for
 * local slot s (its cells take those sizes); a request beyond a record's end
 * returns DCCRGX_EINVAL.  bytes_left: per local slot, the unread bytes of its
 * record.  Nothing else may change the grid between start and finish.
 * save_grid_data does not truncate the file (the reference does not
 * either), so the last record of a file is bounded by the end of the file:
 * bytes after the grid data (an older, longer file at the same path, or the
 * caller's own) count toward that record's bytes_left. */
int dccrgx_start_loading_grid_data(dccrgx_grid* g, const char* path, uint64_t offset, size_t header_bytes);
int dccrgx_continue_loading_grid_data(dccrgx_grid* g, int field_id, const uint64_t* sizes);
int dccrgx_finish_loading_grid_data(dccrgx_grid* g);
int dccrgx_grid_file_bytes_left(dccrgx_grid* g, uint64_t* bytes);

/* ---- partition (pin 5832/5859, unpin 5909, balance_load 1024 and its
 * split form initialize_balance_load 3746 / continue_balance_load 3899 /
 * finish_balance_load 3942).  Collective.  The new owners (make_new_partition
 * 8349-8581) are, each overriding the one before: the native partitioner's
 * (use_partitioner != 0 and load balancing method "RCB", the reference's
 * default Zoltan method 7082: recursive coordinate bisection of the leaves by
 * their centers and weights, computed on the device - parity unpinned against
 * Zoltan, which is absent), an optional export list of this rank (local cells
 * and their new process, a partitioner's Zoltan_LB_Balance export list), and
 * the pins.  Method "NONE" or use_partitioner == 0: only exports and pins move
 * (balance_load(false)).  Cell weights are dropped (1011-1018).  continue
 * moves the payloads of every field (RCCL or the host exchange); finish
 * rebuilds every structure on the device, fetching the new ghost leaves from
 * their owners, and places the arrived payloads. */
int dccrgx_pin(dccrgx_grid* g, uint64_t cell, int process);
int dccrgx_unpin(dccrgx_grid* g, uint64_t cell);
int dccrgx_balance_load(dccrgx_grid* g, int use_partitioner);
int dccrgx_balance_load_to(dccrgx_grid* g, const uint64_t* cells, const int32_t* new_process, size_t n);
int dccrgx_initialize_balance_load(dccrgx_grid* g, int use_partitioner, const uint64_t* cells,
                                   const int32_t* new_process, size_t n);
/* the native partitioner's decision alone, no migration: every local cell
 * (ascending id) and its new process.  Collective. */
int dccrgx_make_new_partition(dccrgx_grid* g, uint64_t* cells, int32_t* new_process, size_t cap, size_t* n);
/* set_load_balancing_method 8223 ("RCB" default, "NONE"; other Zoltan methods
 * are EINVAL) / get_load_balancing_method 8228 (NUL-terminated into out) */
int dccrgx_set_load_balancing_method(dccrgx_grid* g, const char* method);
int dccrgx_get_load_balancing_method(dccrgx_grid* g, char* out, size_t cap);
/* set_cell_weight 6210 (local leaves; ENOTFOUND otherwise; children inherit
 * their parent's weight) / get_cell_weight 6244 (1 when unset, NaN for a
 * cell that is not a local leaf) */
int dccrgx_set_cell_weight(dccrgx_grid* g, uint64_t cell, double weight);
double dccrgx_get_cell_weight(dccrgx_grid* g, uint64_t cell);
int dccrgx_continue_balance_load(dccrgx_grid* g);
/* between initialize_ and finish_balance_load: the cells leaving to
 * (incoming = 0) or arriving from (incoming = 1) `peer`, ascending (the
 * reference's cells_to_send / cells_to_receive during a balance, 3746-3884) */
int dccrgx_get_migration_cells(dccrgx_grid* g, int peer, int incoming, uint64_t* ids, size_t cap, size_t* n);
int dccrgx_finish_balance_load(dccrgx_grid* g);
/* Explicit migration transport (instead of continue_balance_load): the
 * message to / from `peer` = for every field in field order, the payload of
 * each moving cell in ascending id.  pack after initialize, place before
 * finish; *_size gives both byte counts. */
int dccrgx_migration_message_size(dccrgx_grid* g, int peer, size_t* send_bytes, size_t* recv_bytes);
int dccrgx_migration_pack(dccrgx_grid* g, int peer, void* buf, size_t cap);
int dccrgx_migration_place(dccrgx_grid* g, int peer, const void* buf, size_t bytes);

/* ---- fields (replaces Cell_Data + get_mpi_datatype, dccrg_get_cell_datatype.hpp:40-340)
 * transfer != 0: the field is part of update_copies_of_remote_neighbors. */
int dccrgx_add_field(dccrgx_grid* g, const char* name, size_t elem_bytes, int transfer, int* field_id);
int dccrgx_set_field_transfer(dccrgx_grid* g, int field_id, int transfer);
/* the bytes of each element the halo carries: [offset, offset + bytes) (what
 * Cell_Data::get_mpi_datatype describes; default: the whole element) */
int dccrgx_set_field_window(dccrgx_grid* g, int field_id, size_t offset, size_t bytes);
/* the field's device array (slot order).  The pointer stays valid until the
 * next structural change (refinement, balance_load, loading a file).  Writes
 * made through it are seen by every call - the advection sweeps, their
 * time step (dccrgx_advection_max_time_step and its device form) and
 * dccrgx_advection_check_adaptation keep nothing derived from a field whose
 * pointer is out; the library's own bookkeeping of a
 * field's contents (e.g. dccrgx_get_live_neighbors' record that the list
 * field's inner rows are already zero) is reset only when this function is
 * called, so a program that writes through a pointer it fetched earlier
 * fetches it again after such writes. */
int dccrgx_field_device_ptr(dccrgx_grid* g, int field_id, void** ptr);
/* host <-> device copies of whole slot ranges [slot0, slot0+n) */
int dccrgx_field_upload(dccrgx_grid* g, int field_id, size_t slot0, size_t n, const void* host);
int dccrgx_field_download(dccrgx_grid* g, int field_id, size_t slot0, size_t n, void* host);

/* ---- variable-size payloads (a Cell_Data whose get_mpi_datatype describes
 * a different number of bytes per cell, e.g. a std::vector member:
 * tests/variable_data_size/variable_data_size.cpp, variable_neighbour_data.cpp;
 * dccrg_get_cell_datatype.hpp:40-340).  One byte pool over all slots; a new
 * field, new children and new remote copies start empty (the reference
 * default-constructs them).  The halo, migrations (continue_balance_load)
 * and the removed-cell store move every cell's size with its bytes, so a
 * receiver takes the sender's sizes (the reference needs the receiver to
 * size its copies first, variable_neighbour_data.cpp:95-102, 133-145; done
 * that way the bytes are the same).  Grid files and the explicit halo /
 * migration message calls (dccrgx_halo_*, dccrgx_migration_*) refuse them
 * (DCCRGX_EINVAL); the fixed-field calls (dccrgx_field_*) refuse a variable
 * field. */
int dccrgx_add_variable_field(dccrgx_grid* g, const char* name, int transfer, int* field_id);
/* byte sizes of slots [slot0, slot0 + n) */
int dccrgx_variable_field_sizes(dccrgx_grid* g, int field_id, size_t slot0, size_t n, uint64_t* sizes);
/* new byte sizes of slots [slot0, slot0 + n): each cell keeps its first
 * min(old, new) bytes, new bytes are zero (std::vector::resize) */
int dccrgx_variable_field_resize(dccrgx_grid* g, int field_id, size_t slot0, size_t n, const uint64_t* sizes);
/* the concatenated bytes of slots [slot0, slot0 + n); upload needs exactly
 * their current total, download sets *nbytes (DCCRGX_ERANGE when cap is short) */
int dccrgx_variable_field_upload(dccrgx_grid* g, int field_id, size_t slot0, size_t n, const void* bytes,
                                 size_t nbytes);
int dccrgx_variable_field_download(dccrgx_grid* g, int field_id, size_t slot0, size_t n, void* bytes, size_t cap,
                                   size_t* nbytes);
/* device pool and the n_slots + 1 byte offsets (slot s: [off[s], off[s+1])) */
int dccrgx_variable_field_device_ptr(dccrgx_grid* g, int field_id, void** data, const uint64_t** offsets);
/* the removed cells' payloads (order of dccrgx_get_removed_cells): sizes
 * (one per removed cell, may be NULL) and concatenated bytes */
int dccrgx_removed_variable_field_download(dccrgx_grid* g, int field_id, uint64_t* sizes, void* bytes, size_t cap,
                                           size_t* nbytes);
/* ---- particles in cells (tests/particles/simple.cpp) -----------------------
 * get_existing_cell(coordinate) (dccrg.hpp:6316-6336) for n host coordinates
 * (x, y, z each): the smallest leaf known to this process at each one, 0
 * (error_cell) outside the grid or where nothing is known.  The wrap and the
 * indices are Cartesian_Geometry::get_real_coordinate / get_indices
 * (dccrg_cartesian_geometry.hpp:521-607): a coordinate exactly at the grid's
 * end indexes one past the last cell and yields 0, in a periodic dimension
 * too.  Cartesian geometry only (DCCRGX_EINVAL with a stretched block). */
int dccrgx_get_existing_cells_at(dccrgx_grid* g, const double* xyz, size_t n, uint64_t* ids);
/* One step of propagate_particles (simple.cpp:52-97) on the device.  The
 * variable field holds fp64 records of record_doubles (K >= 3) doubles per
 * particle, doubles 0..2 the position, the rest carried along; velocity NULL
 * (K >= 6) takes each particle's velocity from doubles 3..5.  Over the local
 * cells and the copies of remote neighbors: x' = real_coordinate(x + v dt)
 * (product and sum rounded separately) is stored back; a particle whose leaf
 * is its cell stays, one whose leaf is a local cell in neighbors_of of its
 * cell (for a remote copy: a local cell with the copy in neighbors_to) is
 * appended there, any other leaves this process's lists.  A local cell ends
 * with its stayers in their previous order, then the arrivals ordered by
 * (source cell id, index in the source cell); remote copies end empty.
 * stats = {stayed, moved between local cells, arrived from remote copies,
 * handed over (a known remote cell in neighbors_of), lost}.  DCCRGX_EINVAL:
 * a fixed-size field, a cell whose bytes are no multiple of 8 K, K < 3,
 * velocity NULL with K < 6, a stretched geometry block. */
int dccrgx_particles_step(dccrgx_grid* g, int var_field, int record_doubles, const double* velocity, double dt,
                          uint64_t* stats);
/* Particles follow the mesh.  The reference hands a refined parent's data to
 * the user in refined_cell_data (dccrg.hpp:10215-10219) and the removed
 * children's in unrefined_cell_data (10387) and leaves the new cells
 * default-constructed; with this on (record_doubles = K >= 3, 0 turns it off
 * again; off by default) every dccrgx_stop_refining, the one inside
 * dccrgx_advection_adapt included, moves the field's records itself, on the
 * device: a refined local parent's record goes to the leaf of the new mesh
 * that get_existing_cell (6316-6336; the step's point location, Cartesian or
 * stretched) names for its stored position, which is not rewritten; each
 * child holds its records in the parent's order; a record whose leaf is not
 * one of the parent's eight children leaves the lists and is counted lost.
 * The new parent of a merged family receives the removed children's records,
 * ascending child id, each child's in their own order; the removed store
 * (dccrgx_removed_variable_field_download) answers as before.  Cells that
 * stay keep their records, remote copies start empty.  DCCRGX_EINVAL here: a
 * fixed-size field, K of 1 or 2.  DCCRGX_EINVAL from the stop_refining, the
 * mesh and the refine / unrefine requests unchanged: a local cell whose bytes
 * are no multiple of 8 K, a stretched geometry block without coordinates. */
int dccrgx_particles_follow_mesh(dccrgx_grid* g, int var_field, int record_doubles);
/* out = {records moved to children, records moved to parents, lost} of this
 * process in the last dccrgx_stop_refining */
int dccrgx_particles_adapt_stats(dccrgx_grid* g, int var_field, uint64_t out[3]);
/* Particles <-> cell fields.  A record p held by leaf s gives leaf c the
 * share W(p, c).  shape 0 (NGP): 1 for c == s, 0 otherwise; the position is
 * not read.  shape 1 (CIC over leaves, Cartesian geometry): the cloud is a box
 * the size of s centred on the particle, W the fraction of its volume inside
 * c; the receivers are s and the distinct leaves of neighbors_of(s).  Every
 * product, quotient and sum is one IEEE operation, in this order, per
 * dimension d: a cell of index i (finest units) and level l has
 * lo = start + (double(i) * l0) / 2^R (dccrgx_geometry_fill's low),
 * L = l0 * (1 / 2^l), hi = lo + L; xc = min(max(x, lo_s), hi_s) (a record
 * outside its cell is clamped into it); a = xc - L_s / 2, b = xc + L_s / 2;
 * o_k = max(0, min(b, hi_c + k P) - max(a, lo_c + k P)) with
 * P = double(length_d) * l0_d, k = -1, 0, +1 in a periodic dimension and 0
 * only otherwise, o = (o_-1 + o_0) + o_+1; f_d = o / L_s.  W = (f_x f_y) f_z.
 * The share of a cloud past a non-periodic face is dropped.
 *
 * deposit: for every local cell c, out[c] = the sum of q_p W(p, c) over the
 * records of c and of the distinct leaves of neighbors_of(c), the copies of
 * remote neighbors included; q_p = record[weight_double] (3 <= weight_double
 * < K), or 1 with weight_double == -1.  per_volume != 0 divides the sum by
 * (lx ly) lz, dccrgx_geometry_fill's lengths, Cartesian or stretched.
 * out_field is a fixed fp64 field; its remote-copy slots are not written.  No
 * atomic decides a sum: two calls on one state give bitwise equal fields;
 * only the order of a sum is unspecified.  DCCRGX_EINVAL: a fixed-size
 * var_field, an out_field that is no fixed 8-byte field, K < 3, a cell whose
 * bytes are no multiple of 8 K, weight_double out of range, shape not 0 or 1,
 * shape 1 with neighborhood length 0 or a stretched geometry (set or a file's
 * block), per_volume with a stretched block without coordinates. */
int dccrgx_particles_deposit(dccrgx_grid* g, int var_field, int record_doubles, int shape, int weight_double,
                             int out_field, int per_volume);
/* gather: for every record p of a local cell s,
 * record[first_double + j] = the sum of W(p, c) F_j[c] over s and the
 * distinct leaves of neighbors_of(s), j < n; F_j = cell_fields[j], fixed fp64
 * fields whose remote copies are read (update them first).  No
 * renormalisation at an open face: a field of ones gathers the share of the
 * cloud inside the grid.  The positions, every other double and the records
 * of remote copies are not written.  DCCRGX_EINVAL as for deposit, and unless
 * 3 <= first_double, first_double + n <= K, n >= 1. */
int dccrgx_particles_gather(dccrgx_grid* g, int var_field, int record_doubles, int shape, const int* cell_fields,
                            int n, int first_double);
/* accelerate: for every record of a local cell, k = factor * q with
 * q = record[weight_double], or q = 1 with weight_double == -1 (then
 * k = factor), and record[3 + j] = record[3 + j] + k * record[first_double + j]
 * for j = 0, 1, 2, the product rounded first and then the sum.  Nothing else of
 * a record and no record of a remote copy is written.  DCCRGX_EINVAL as for
 * gather (no shape is taken), and unless 6 <= first_double,
 * first_double + 3 <= K, and weight_double is -1 or in [6, K) outside
 * [first_double, first_double + 3). */
int dccrgx_particles_accelerate(dccrgx_grid* g, int var_field, int record_doubles, int first_double,
                                int weight_double, double factor);
/* deposit_moments: n moments of the records in one walk of the deposit.  For
 * every local cell c and j < n, out_fields[j][c] = the sum of m_j(p) W(p, c)
 * over the records of c and of the distinct leaves of neighbors_of(c), the
 * copies of remote neighbors included.  W is the deposit's (shape 0: 1 for the
 * record's own cell; shape 1: the cloud's share), formed once per (record,
 * receiver) and used by all moments.  m_j(p) = (q_p * u) * v with q_p as in
 * deposit (record[weight_double], or 1 with -1), u = record[factors[2 j]],
 * v = record[factors[2 j + 1]]; a factor of -1 stands for 1.0.  q_p * u is one
 * IEEE product, the product with v the next, then term = m_j * W, then the
 * sum.  (-1, -1) is the charge, (3, -1) the x-current q v_x, (3, 4) the
 * pressure component q v_x v_y.  The records are summed in deposit's order
 * (the same lanes take the same records, the same shuffle tree adds them), so
 * an output with factors (-1, -1) is bitwise what dccrgx_particles_deposit
 * writes for the same weight_double, shape and per_volume, wherever it stands
 * in the list.  per_volume divides each sum by (lx ly) lz as deposit does; the
 * outputs' remote-copy slots are not written; with no records the local slots
 * of every output are zeroed; no atomic decides a sum, so two calls on one
 * state give bitwise equal fields.  DCCRGX_EINVAL: everything deposit refuses
 * (shape 1 with neighborhood length 0 or a stretched geometry included), n
 * outside 1 .. 16, a factor that is neither -1 nor in [3, K), an output that
 * is no fixed 8-byte field, two equal outputs. */
int dccrgx_particles_deposit_moments(dccrgx_grid* g, int var_field, int record_doubles, int shape, int weight_double,
                                     const int* factors /* 2 n */, const int* out_fields /* n */, int n,
                                     int per_volume);
/* boris: the Boris kick of every record of a local cell.  v = record[3 .. 5],
 * E = record[e_first ..], B = record[b_first ..] (three doubles each),
 * h = factor * q with q = record[weight_double], or h = factor with
 * weight_double == -1; the caller passes factor = dt / 2m.  Each product,
 * quotient, sum and difference is rounded on its own, in this order (j = 0,
 * 1, 2):
 *   hE_j = h * E_j;   vm_j = v_j + hE_j;   t_j = h * B_j
 *   t2 = (t_0 * t_0 + t_1 * t_1) + t_2 * t_2;   den = 1.0 + t2
 *   s_j = (2.0 * t_j) / den
 *   c = vm x t:  c_0 = vm_1 * t_2 - vm_2 * t_1, c_1 = vm_2 * t_0 - vm_0 * t_2,
 *                c_2 = vm_0 * t_1 - vm_1 * t_0;          vp_j = vm_j + c_j
 *   d = vp x s   (the same form);                        vq_j = vm_j + d_j
 *   v_j = vq_j + hE_j
 * Nothing else of a record and no record of a remote copy is written.
 * DCCRGX_EINVAL as for accelerate, and unless 6 <= e_first, e_first + 3 <= K,
 * 6 <= b_first, b_first + 3 <= K, the two ranges do not overlap, and
 * weight_double is -1 or in [6, K) outside both. */
int dccrgx_particles_boris(dccrgx_grid* g, int var_field, int record_doubles, int e_first, int b_first,
                           int weight_double, double factor);
/* create: new records are appended to the lists of the local cells, on the
 * device.  Every value is a function of (seed, cell id, index i among the
 * cell's new records, double j) alone: not of the slot, the number of
 * processes, what the lists hold or the launch; two calls give equal bits.
 *
 * Random numbers: Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57, key
 * increments 0x9E3779B9, 0xBB67AE85), key = (seed's low word, seed's high
 * word), counter = (id's low word, id's high word, i, block number).  A
 * block's words w0..w3 give two uniforms in [0, 1):
 * first = double((uint64(w0) << 21) | (w1 >> 11)) * 2^-53, second the same
 * from w2, w3.  (Known answer: counter 0,0,0,0 under key 0,0 gives
 * 6627e8d5 e169c58d bc57ac4c 9b00dbd8.)
 *
 * Counts, for every local cell c: v = count with count_field == -1, else
 * v = count * F[c] (one product; F a fixed fp64 field); round_random == 0:
 * n_c = floor(v); round_random == 1: n_c = floor(v + u), one rounded sum, u
 * the first uniform of the block with counter (id low, id high, 0xFFFFFFFF,
 * 0xFFFFFFFF).  A v that is NaN, negative or >= 2^31 in any local cell is
 * DCCRGX_EINVAL, found on the device with nothing changed; dccrgx_last_error
 * names the cell.
 *
 * Placement: a cell's existing records keep their bits and their order, the
 * n_c new ones follow, i = 0 .. n_c - 1.  Remote copies receive nothing and
 * keep their bytes.  *created = the process's total; a total of 0 changes
 * nothing (no write is recorded).
 *
 * Doubles 0..2, the position (their recipe entries are ignored): with center
 * and L what dccrgx_geometry_fill writes for the cell (Cartesian or
 * stretched), u_x, u_y = first, second of block 0, u_z = first of block 1:
 *   h = u - 0.5 (exact);  x = center + h * L (one product, one sum)
 *   lo = center - L / 2;  hi = center + L / 2
 *   stored: min(max(x, lo), pred(hi)), pred the next double towards -inf,
 * so the position is in [lo, hi) whatever the rounding.
 *
 * Double j >= 3, recipe_i[3 j ..] = (kind, base_field, spread_field),
 * recipe_d[2 j ..] = (a, b), block j:  base = a with base_field == -1, else
 * a * Fa[c];  spread = b with spread_field == -1, else b * Fb[c] (one product
 * each; fixed fp64 fields).
 *   kind 0 (constant): base; no block is computed, spread is not formed
 *   kind 1 (uniform):  base + spread * first
 *   kind 2 (normal):   base + spread * z with
 *       w = 1.0 - first (exact, in (0, 1]);  t = -2.0 * log(w);  r = sqrt(t)
 *       theta = 6.283185307179586 * second;  z = r * cos(theta)
 * each one operation, the product rounded before the sum; log and cos are the
 * device library's, sqrt is correctly rounded.  A weight a * density[c], a
 * drift Fa[c] (a = 1) and a thermal speed b * Fb[c] are all of this form.
 * A cell field whose device pointer was handed out is read as it is.
 *
 * DCCRGX_EINVAL: a fixed-size var_field; K < 3; a local cell whose bytes are
 * no multiple of 8 K; a kind outside 0..2 for j >= 3; a field id (count_field,
 * or a base_field / spread_field of j >= 3) that is neither -1 nor a fixed
 * 8-byte field; round_random not 0 or 1; count not finite; more than 2^31 - 1
 * records on the process afterwards; a stretched geometry block without
 * coordinates (as for per_volume). */
int dccrgx_particles_create(dccrgx_grid* g, int var_field, int record_doubles /* K */, int count_field, double count,
                            int round_random, const int* recipe_i /* 3 K: kind, base_field, spread_field */,
                            const double* recipe_d /* 2 K: a, b */, uint64_t seed, uint64_t* created);
/* remove: records leave the lists of the local cells, on the device; the
 * counterpart of create.  Remote copies keep their bytes and sizes.
 *
 * The decision, for the record with index i in the list of local cell c as
 * the list stands before the call: it is removed by the first stage that
 * holds, else kept.
 *   1. mask: mask_field != -1 is a fixed fp64 field M; removed when
 *      M[c] != 0.0 (a NaN absorbs, -0.0 does not).
 *   2. tests t = 0 .. n_tests - 1 (0 <= n_tests <= 8): x = record[test_i[2 t]]
 *      (any double 0 <= j < K), in = (lo_t <= x) && (x < hi_t) with
 *      lo_t, hi_t = test_d[2 t], test_d[2 t + 1]: a NaN x is not in, infinite
 *      bounds give one-sided tests, lo == hi is the empty interval.  Mode
 *      test_i[2 t + 1]: 0 (keep inside) removes when !in, 1 (drop inside)
 *      removes when in.
 *   3. chance, active when prob_field != -1 || prob != 0.0: p_c = prob, or
 *      prob * F[c] (one product; F a fixed fp64 field).  u = the first uniform
 *      (create's words-to-double rule) of the Philox4x32-10 block with key =
 *      (seed's low word, seed's high word) and counter (id low, id high, i,
 *      0xFFFFFFFE); removed when u < p_c, so p_c <= 0 or NaN removes nothing
 *      and p_c >= 1 everything.  i is the index before the call whatever
 *      stages 1 and 2 removed; no block is computed for a record an earlier
 *      stage removed.  The verdict is a function of (seed, cell id, i, the
 *      record, the cell's field values) alone.
 * rescale != 0 (needs weight_double != -1): a record that reaches stage 3 and
 * is kept, in a cell with 0 < p_c < 1, gets
 *   rest = 1.0 - p_c;  record[w] = record[w] / rest
 * (one difference, one quotient).  Nothing else of a kept record is written;
 * a cell's kept records keep their bits and their relative order.
 *
 * Tallies j = 0 .. n_tally - 1 (0 <= n_tally <= 4), of a removed record:
 *   m_j = (q * u) * v, q = record[weight_double] (1.0 with -1), u, v =
 *   record[tally_factors[2 j]], record[tally_factors[2 j + 1]] (-1: 1.0), each
 *   product rounded as in dccrgx_particles_deposit_moments;
 *   T_j[c] = T_j[c] + S_j(c), S_j(c) the sum of m_j over the records removed
 *   from c by any stage, T_j the fixed fp64 field tally_fields[j].  The order
 *   of the sum is unspecified but fixed (no atomic decides it): two calls on
 *   equal states give equal bits.  A cell that loses no record is not written;
 *   remote-copy slots never are.  Factors (-1, -1) collect the absorbed
 *   charge, (3, -1) a momentum, (3, 3) an energy component.
 *
 * into_field: -1 discards the removed records.  Otherwise another variable
 * field whose local cells hold whole records of the same K: the records
 * removed from c are appended behind c's records there, in the order they had
 * in the source list, bits unchanged.  Its remote copies are untouched.
 *
 * stats = {kept, removed by mask, removed by a test, removed by chance}, the
 * totals of this process's local cells.  A call that removes nothing and
 * rescales nothing changes nothing (no write is recorded, no pool is built).
 * A field with no pool, or no local cells: zeros.
 *
 * DCCRGX_EINVAL, before any change and with stats untouched: a fixed-size
 * var_field or into_field; K < 3; a local cell of either pool whose bytes are
 * no multiple of 8 K; n_tests outside 0..8; a tested double outside [0, K); a
 * mode other than 0, 1; a NaN lo or hi; a mask_field, prob_field or tally
 * field that is neither -1 (where allowed) nor a fixed 8-byte field; prob not
 * finite; rescale without weight_double; weight_double neither -1 nor in
 * [3, K); a tally factor neither -1 nor in [3, K); n_tally outside 0..4; two
 * equal tally fields; a tally field equal to mask_field or prob_field;
 * into_field == var_field; more than 2^31 - 1 records in into_field
 * afterwards. */
int dccrgx_particles_remove(dccrgx_grid* g, int var_field, int record_doubles /* K */,
                            const int* test_i /* 2 n_tests: double, mode */,
                            const double* test_d /* 2 n_tests: lo, hi */, int n_tests, int mask_field, int prob_field,
                            double prob, uint64_t seed, int rescale, int weight_double,
                            const int* tally_factors /* 2 n_tally */, const int* tally_fields /* n_tally */,
                            int n_tally, int into_field, uint64_t stats[4]);
/* The cell-centred gradient of the fixed fp64 field in_field over the leaves:
 * out_fields[d] (fixed fp64 fields, -1: component not wanted) of every local
 * cell of `region` (DCCRGX_REGION_*; inner then outer writes the bits of all)
 * = scale * grad_d.  The remote copies of in_field are read (update them
 * first); remote-copy slots of the outputs are never written.  The operator is
 * the first-derivative counterpart of dccrgx_poisson_cache's factors
 * (set_scaling_factor 696-819): the same centre distances and three-point
 * stencil per dimension, so that on a periodic uniform grid the sum over cells
 * of (A phi)(grad_d phi) is zero.  Every product, quotient, sum and difference
 * is one IEEE operation in this order.  For a local leaf c and dimension d:
 * hc = L_c,d / 2 with L the length dccrgx_poisson_cache uses (Cartesian
 * l0_d * (1 / 2^level); stretched (c[i + 1] - c[i]) / 2^level from the cell's
 * own level-0 index i along d; a grid that holds only a stretched file block
 * without coordinates sees each dimension's start and first cell length).  A
 * side has a neighbor unless the cell has no face neighbor there (a grid edge
 * of a non-periodic dimension); then h = hc + L_n,d / 2 with the neighbor's
 * own length and v = in[n], or for four finer neighbors their sum (in an
 * unspecified order) divided by 4.0.  Both sides: tot = h_pos + h_neg,
 * a = h_neg / (h_pos * tot), b = h_pos / (h_neg * tot),
 * grad = a * (v_pos - v_c) + b * (v_c - v_neg).  Only the + side:
 * grad = (v_pos - v_c) / h_pos; only the - side: (v_c - v_neg) / h_neg;
 * neither: 0.  A cell that is its own periodic neighbor gets 0 from the same
 * formula.  The Poisson solver's skip / boundary classification is not
 * consulted: every leaf takes part.  DCCRGX_EINVAL: a variable-size field or
 * one that is not 8 bytes wide, an output equal to the input or to another
 * output, all three outputs -1, a bad region. */
int dccrgx_gradient(dccrgx_grid* g, int in_field, const int out_fields[3], double scale, int region);
/* The curl and the divergence of the three fixed fp64 fields in_fields =
 * (F_0, F_1, F_2) over the leaves, and y = y + a x on two such fields.  Let
 * D_d(F)[c] be exactly the value `grad` of dccrgx_gradient's contract for the
 * input F, the local leaf c and the dimension d, before the scaling: the same
 * lengths, the same side rules (both sides, only +, only -, neither: 0), and
 * the four values of a finer face summed as ((a0 + a1) + (a2 + a3)) / 4.0 in
 * the face's stored order, which is the order dccrgx_gradient uses.  Every
 * step below is one IEEE operation, in this order, so the results are bitwise
 * what a caller combines from dccrgx_gradient's outputs with scale 1.0.
 * curl:        r_0 = D_1(F_2) - D_2(F_1);  r_1 = D_2(F_0) - D_0(F_2);
 *              r_2 = D_0(F_1) - D_1(F_0);  t_k = scale * r_k;
 *              out_fields[k][c] = t_k, or with accumulate != 0
 *              out_fields[k][c] + t_k.  out_fields[k] == -1: the component is
 *              not wanted and not touched; at least one must be wanted.
 * divergence:  r = (D_0(F_0) + D_1(F_1)) + D_2(F_2);  t = scale * r;
 *              out_field[c] = t, or out_field[c] + t.
 * field_axpy:  y[c] = y[c] + (a * x[c]): the product is rounded, then the sum.
 * Every local cell of `region` is written (DCCRGX_REGION_*; inner then outer
 * writes the bits of all, each only its own slots).  The remote copies of the
 * inputs are read (update them first); remote-copy slots of an output or of y
 * are never written.  The three inputs need not be distinct fields.  The
 * Poisson solver's classification is not consulted.  DCCRGX_EINVAL, checked
 * before the first write: a variable-size field, one that is not 8 bytes wide,
 * an invalid field id, an output equal to an input or to another output, all
 * three curl outputs -1, a bad region, x_field == y_field. */
int dccrgx_curl(dccrgx_grid* g, const int in_fields[3], const int out_fields[3], double scale, int accumulate,
                int region);
int dccrgx_divergence(dccrgx_grid* g, const int in_fields[3], int out_field, double scale, int accumulate,
                      int region);
int dccrgx_field_axpy(dccrgx_grid* g, int y_field, double a, int x_field, int region);

/* Cell fields follow the mesh.  The reference gives a new child a copy of its
 * parent's payload and leaves the parent of a merged family default-
 * constructed (execute_refines 10104-10554; the user is handed
 * refined_cell_data and unrefined_cell_data).  With a mode other than OFF every
 * dccrgx_stop_refining, the one inside dccrgx_advection_adapt and induced
 * refines included, restricts and prolongs the local cells of the fixed fp64
 * field field_id itself, on the device.  The mode is per field, starts OFF and
 * holds until it is changed: it survives stop_refining, balance_load and
 * grid-file loads.  Every product, quotient, sum and difference below is one
 * IEEE fp64 operation in the stated order (no contraction).
 *   DCCRGX_FOLLOW_OFF     the behaviour described above, bit for bit
 *   DCCRGX_FOLLOW_MEAN    an intensive quantity (phi, E, B, a density)
 *   DCCRGX_FOLLOW_SUM     an extensive quantity (a charge or a count per cell)
 *   DCCRGX_FOLLOW_LINEAR  MEAN's restriction, limited linear prolongation
 * Merged parent: its eight children c_0 .. c_7 in ascending id, their payloads
 * from the removed store (which holds the children of other processes too and
 * answers as before).  MEAN and LINEAR: acc = 0; for k: acc = acc + c_k / 8.0.
 * SUM: acc = 0; for k: acc = acc + c_k.  Children are of equal volume under
 * both geometries (a stretched level-0 cell is split evenly), so the plain mean
 * is the volume-weighted one.
 * New child of a refined local parent of value v.  MEAN: v.  SUM: v * 0.125.
 * LINEAR, from the old mesh and the old values, the field's remote copies
 * included (update them first, as for dccrgx_gradient): for d = 0, 1, 2,
 * g_d = the value `grad` of dccrgx_gradient's contract for this field, cell and
 * dimension, before the scaling; q_d = L_d * 0.25 with L_d the length that
 * contract uses; e_d = g_d * q_d.  Delta = (|e_0| + |e_1|) + |e_2|.  m and M
 * are the minimum and the maximum of v and of the value of every face-neighbor
 * leaf of the parent: each of the four cells of a finer face counts on its own,
 * a missing side counts for nothing.  alpha = 1.0; if Delta > 0:
 * up = (M - v) / Delta; dn = (v - m) / Delta; alpha = min(1.0, min(up, dn)).
 * t_d = alpha * e_d.  Child k in ascending id has b_d = bit d of k and
 * s_d = +1 if b_d is set, -1 otherwise; its value is
 * ((v + s_0 t_0) + s_1 t_1) + s_2 t_2.
 * Consequences: a local extremum is injected (alpha = 0), and so is a cell
 * whose only neighbor along the one direction of variation is missing at an
 * open edge; the children stay inside [m, M] up to rounding, so a non-negative
 * field stays non-negative; the mean of the eight children is v up to rounding.
 * Everything else is as with OFF: cells that stay keep their bits, remote-copy
 * slots are carried as before (update them before reading them), a field the
 * call itself rewrites (dccrgx_advection_adapt's density, velocities and
 * lengths) keeps that call's rule whatever its mode.
 * DCCRGX_EINVAL: a variable-size field, a field that is not 8 bytes wide, a bad
 * field id, a bad mode. */
#define DCCRGX_FOLLOW_OFF 0
#define DCCRGX_FOLLOW_MEAN 1
#define DCCRGX_FOLLOW_SUM 2
#define DCCRGX_FOLLOW_LINEAR 3
int dccrgx_field_follow_mesh(dccrgx_grid* g, int field_id, int mode);
int dccrgx_field_follow_mode(dccrgx_grid* g, int field_id, int* mode);

/* Reductions on the device: the scalars of a cycle (field energy, total
 * charge, kinetic energy, max |v|, max |div B|) without the download of a
 * field.  One call computes n = 1 .. 16 terms in one pass; terms holds three
 * ints per term: the operation and two factors.  Every step is one IEEE
 * operation.
 * field_reduce, term j over the local cells c of `region` (DCCRGX_REGION_*;
 * remote-copy slots are never read): t = a[c] * b[c] with a, b the fixed fp64
 * fields terms[3 j + 1], terms[3 j + 2]; a field id of -1 stands for 1.0, so
 * (a, -1) is a[c] itself and (-1, -1) is 1.0; a == b is a square.  With
 * by_volume != 0 a SUM term becomes t * V_c, V_c = (lx ly) lz of
 * dccrgx_geometry_fill's lengths, the volume the deposit's per_volume divides
 * by, Cartesian or stretched; by_volume does not touch the other operations.
 * particles_reduce, term j over the records p of the local cells (records of
 * remote copies are not read): m = (q_p * u) * v, exactly
 * dccrgx_particles_deposit_moments' m_j: q_p = record[weight_double], or 1
 * with -1; u = record[terms[3 j + 1]], v = record[terms[3 j + 2]], doubles in
 * [3, record_doubles) or -1 for 1.0.  Weight -1 and (-1, -1) SUM is the record
 * count as a double, (-1, -1) SUM the total charge, (3, -1) SUM the
 * x-momentum, (3, 3) + (4, 4) + (5, 5) twice the kinetic energy, weight -1
 * and (3, -1) MAX_ABS max |v_x|.
 * SUM adds the terms in an unspecified but fixed order (a function of the
 * number of elements and of distinct fields only); no atomic decides a sum, so
 * two calls on one state give bitwise equal results, in the host form and the
 * device form alike.  MIN and MAX are taken over the terms, MAX_ABS over
 * fabs(term); they are exact.  Over no elements the results are SUM +0.0,
 * MIN +inf, MAX -inf, MAX_ABS +0.0.  A NaN among the inputs propagates through
 * SUM per IEEE; the result of the three extrema is then unspecified (the
 * comparisons keep their first operand on NaN).
 * collective == 0: this process's values only (works on a detached view).
 * collective != 0: every process calls; the processes' values are all-gathered
 * on the device and combined in rank order (MAX_ABS as MAX), so every process
 * gets the same bits.
 * The _device form writes the n doubles d_out in device memory, queued on the
 * compute stream (dccrgx_compute_stream): field_reduce_device never waits on
 * the host (over RCCL; a host exchange function stages the collective through
 * the host); particles_reduce_device first reads back the check of the cells'
 * byte counts and the number of local records, as every particle call does,
 * and waits for nothing after that.  The host form is the device form
 * followed by one synchronising copy of n doubles: the same bits.
 * DCCRGX_EINVAL, before any work and with the output untouched: n outside
 * 1 .. 16, an unknown operation, a field that is variable-size or not 8 bytes
 * wide, an invalid id other than -1, a bad region, by_volume while the grid
 * holds a stretched geometry block without coordinates (deposit's rule),
 * collective on several processes without a communicator, a null pointer;
 * for particles everything deposit_moments refuses of var_field,
 * record_doubles, the cells' byte counts, weight_double and the factors. */
#define DCCRGX_REDUCE_SUM 0
#define DCCRGX_REDUCE_MIN 1
#define DCCRGX_REDUCE_MAX 2
#define DCCRGX_REDUCE_MAX_ABS 3
int dccrgx_field_reduce(dccrgx_grid* g, const int* terms /* 3 n: op, a_field, b_field */, int n, int by_volume,
                        int region, int collective, double* out /* n, host */);
int dccrgx_field_reduce_device(dccrgx_grid* g, const int* terms /* 3 n */, int n, int by_volume, int region,
                               int collective, double* d_out /* n, device */);
int dccrgx_particles_reduce(dccrgx_grid* g, int var_field, int record_doubles, int weight_double,
                            const int* terms /* 3 n: op, u, v */, int n, int collective, double* out /* n, host */);
int dccrgx_particles_reduce_device(dccrgx_grid* g, int var_field, int record_doubles, int weight_double,
                                   const int* terms /* 3 n */, int n, int collective, double* d_out /* n, device */);

/* set_send_single_cells 6677 / get_send_single_cells 6684: one message per
 * cell (tag = position + 1) instead of one per process.  On, the remote
 * neighbor updates put each cell's fixed-size payload on the wire as its own
 * message (per cell in the send list's order, a cell's fields in field
 * order; RCCL posts them in that order, which is how its point-to-point
 * matches them); off, one message per peer and field.  Variable-size fields,
 * migrations and removed-cell payloads keep one message per peer.  The
 * received payloads are identical either way. */
int dccrgx_set_send_single_cells(dccrgx_grid* g, int on);
int dccrgx_get_send_single_cells(dccrgx_grid* g, int* on);

/* ---- halo (update_copies_of_remote_neighbors 966-1000 and its split form
 * start_remote_neighbor_copy_updates 5010, wait_* 5267-5367) ------------- */
int dccrgx_update_copies_of_remote_neighbors(dccrgx_grid* g);
int dccrgx_start_remote_neighbor_copy_updates(dccrgx_grid* g);
int dccrgx_wait_remote_neighbor_copy_update_receives(dccrgx_grid* g);
int dccrgx_wait_remote_neighbor_copy_update_sends(dccrgx_grid* g);
int dccrgx_wait_remote_neighbor_copy_updates(dccrgx_grid* g);
/* Explicit halo transport of one neighborhood (DCCRGX_DEFAULT_HOOD or a user
 * id): the message to / from `peer` = for every transferred field in field
 * order, the window bytes of each cell of cells_to_send / cells_to_receive
 * in ascending id (the wire order of start_user_data_sends / _receives
 * 10587-10997).  pack gathers from the device fields into a host buffer,
 * place scatters a received message into the halo copies. */
int dccrgx_halo_message_size(dccrgx_grid* g, int hood_id, int peer, size_t* send_bytes, size_t* recv_bytes);
int dccrgx_halo_pack(dccrgx_grid* g, int hood_id, int peer, void* buf, size_t cap);
int dccrgx_halo_place(dccrgx_grid* g, int hood_id, int peer, const void* buf, size_t bytes);

/* ---- built-in sweeps (user stencils of tests/ and examples/) ------------- */
/* game of life over cell.neighbors_of (examples/game_of_life.cpp:54-79,
 * tests/game_of_life/scalability3d.cpp:130-165); state is a uint32 field.
 * Reads state, writes the next state into a scratch buffer; the field's
 * device pointer is swapped when dccrgx_gol_commit is called. */
int dccrgx_gol_step(dccrgx_grid* g, int state_field, int region);
int dccrgx_gol_commit(dccrgx_grid* g, int state_field);

/* Game of life on a refined grid emulating the unrefined game:
 * get_live_neighbors, tests/game_of_life/solve.hpp:37-170, split at its halo.
 * phase 0 (collect, 46-110): list_field[cell] = the distinct level-0 parents
 * of live neighbors (neighbors_of order, own parent skipped), error_cell (0)
 * padded; phase 1 (spread + rule, 113-167): merge the lists of same-parent
 * neighbors, count, update state in place.  Between the phases the caller
 * runs update_copies_of_remote_neighbors (both fields transferred).
 * list_field: 64-byte elements (8 x uint64 = Cell_Data::data[1..8]).
 * DCCRGX_EINVAL where the reference aborts (list overflow, siblings
 * disagreeing on their state). */
int dccrgx_gol_amr(dccrgx_grid* g, int phase, int state_field, int list_field, int region);
/* One whole turn of get_live_neighbors (solve.hpp:37-170): collect, the halo
 * (update_copies_of_remote_neighbors, every transferred field), spread + rule,
 * and every local list left error_cell-cleared as the reference's rule loop
 * leaves it (163).  Inside the turn the collected lists live in the kernels'
 * per-cell bit masks; list_field receives only the lists other processes
 * read (the outer cells'), for the halo, and those are cleared at the end.
 * Same states as phase 0 + halo + phase 1; same errors. */
int dccrgx_get_live_neighbors(dccrgx_grid* g, int state_field, int list_field);
/* first-order upwind advection over face neighbors, flux + apply fused
 * (tests/advection/solve.hpp:44-279).  fields: density, vx, vy, vz, lx, ly, lz
 * (all fp64).  Writes the new density into a scratch buffer; commit swaps. */
int dccrgx_advection_step(dccrgx_grid* g, const int fields[7], double dt, int region);
int dccrgx_advection_commit(dccrgx_grid* g, int density_field);
/* advection helpers: initial condition (tests/advection/initialize.hpp:36-82)
 * and max_time_step (solve.hpp:289-333, local part; caller reduces MIN) */
int dccrgx_advection_initialize(dccrgx_grid* g, const int fields[7]);
int dccrgx_advection_max_time_step(dccrgx_grid* g, const int fields[7], double* local_min);
/* the same, reduced over all processes (MIN in rank order, solve.hpp:317),
 * written to DEVICE memory d_out[0] in stream order on the compute stream:
 * no host synchronization over RCCL, so an adaptive loop can take dt
 * without a round trip (ABI 8) */
int dccrgx_advection_max_time_step_device(dccrgx_grid* g, const int fields[7], double* d_out);
/* refine candidates of check_for_adaptation (tests/advection/adapter.hpp:47-178):
 * local cells whose max face relative difference exceeds (lvl+1)*diff_increase */
int dccrgx_advection_refine_candidates(dccrgx_grid* g, int density_field, double diff_increase,
                                       double diff_threshold, uint64_t* out, size_t cap, size_t* n);

/* grid adaptation of tests/advection (adapter.hpp): check_adaptation
 * (47-178) classifies every local cell by the relative density difference to
 * its face neighbors and issues the refine / dont_unrefine / unrefine
 * requests adapt_grid would (counts: the three numbers accepted); call it
 * between the step and the commit, as 2d.cpp does before apply_fluxes.
 * adapt (232-309, collective): stop_refining, merged parents get their
 * children's mean density, velocities and lengths of every local cell are
 * reset, and all seven fields go through one halo (transfer_all_data).
 * out: created and removed cells of this rank. */
int dccrgx_advection_check_adaptation(dccrgx_grid* g, int density_field, double diff_increase,
                                      double diff_threshold, double unrefine_sensitivity, uint64_t counts[3]);
int dccrgx_advection_adapt(dccrgx_grid* g, const int fields[7], uint64_t out[2]);
/* data layout of the advection sweep (built on first use): out[0] tile size,
 * [1] tiles, [2] distinct out-of-tile face neighbors summed over the tiles,
 * [3] largest per-tile count, [4] finer faces, [5] face-neighbor entries
 * (get_face_neighbors_of summed over local cells), [6] algorithmic HBM bytes
 * of one sweep over all local cells as SURVEY §8(d) fixes them (64 B per cell
 * + 4 B per face entry + 4 B per row pointer), [7] the 64 B-per-cell core
 * alone, [8] regular tiles (aligned uniform boxes swept without face rows),
 * [9] cells in regular tiles, [10] out-of-tile face neighbors of the regular
 * tiles (64 per existing side), [11] the bytes the sweep kernels need per
 * sweep, each value read once: the 64-B core, per cell of an irregular tile
 * its 12 B of face codes, per out-of-tile neighbor its density, three
 * lengths and the velocity along the face (40 B; 32 B with the experimental
 * neighbor records) plus 4 B of list entry in an irregular tile, 8 B per
 * finer face, 32 B per tile record (ABI 9: out[12]).  When the sweep of the
 * fields last passed to an advection call takes the cell lengths from the
 * per-level table (dccrgx_advection_length_source), [11] counts 40 B per own
 * cell (41 B in an irregular tile: its level byte) and 16 B per out-of-tile
 * neighbor (density and the velocity along the face; + its level byte in an
 * irregular tile).  When that sweep also takes a velocity component from a
 * kernel argument (dccrgx_advection_velocity_source), [11] counts per uniform
 * component 8 B less per own cell and per out-of-tile neighbor of a regular
 * tile across a side of that axis, and 8 B less per out-of-tile neighbor
 * entry of an irregular tile every axis of whose faces is uniform (counted on
 * the device from the entries' axis bits).  [6] and [7] stay SURVEY's
 * definition.
 * No reference counterpart (roofline introspection). */
int dccrgx_advection_layout(dccrgx_grid* g, uint64_t out[12]);

/* How the tile sweep of the fields last passed to an advection call launches
 * its two persistent kernels: out[0] the blocks per CU the regular tiles'
 * kernel is launched with (its grid is min(CUs x that, tiles rounded up to
 * 8)), [1] the blocks per CU the runtime's occupancy query reports now for
 * that kernel at the dynamic LDS size it is launched with, [2] that size in
 * bytes; [3..5] the same for the kernel of all other tiles.  The sweeps that
 * take the cell lengths from the per-level table size their grids by the
 * query, so [0] == [1] and [3] == [4] there; the field-reading sweeps and the
 * experiment variants are launched with two.  No reference counterpart. */
int dccrgx_advection_occupancy(dccrgx_grid* g, uint64_t out[6]);

/* Where the tile sweeps of fields fids (density, vx, vy, vz, lx, ly, lz) take
 * the cell lengths from: *out = 1 the per-level table l0[d] * 2^-level (every
 * slot's three lengths, remote copies included, were compared bitwise with
 * their level's row by a device pass, cached until the tiles, the geometry or
 * the length fields change), 0 the length fields (the lengths differ
 * somewhere, a length field's device pointer is out, a stretched geometry
 * block is held, or DCCRGX_LEN_TABLE=0).  The densities are bitwise the same
 * either way.  No reference counterpart. */
int dccrgx_advection_length_source(dccrgx_grid* g, const int fids[7], int* out);

/* Which velocity components the tile sweeps of fields fids take from a kernel
 * argument instead of reading them: bit a of *mask (0 vx, 1 vy, 2 vz) is set
 * when every slot of that field, remote copies included, holds one 64-bit
 * pattern (-0.0 among +0.0 is not uniform, equal NaN patterns are), found by
 * one device pass and cached until the tiles or one of the three fields
 * change.  0: the sweeps read the three fields - a component differs
 * somewhere, a velocity field's device pointer is out, the sweeps read the
 * length fields (dccrgx_advection_length_source is 0), the velocities were
 * found rewritten before two sweeps in a row (no pass is made then until a
 * sweep finds them unwritten), or DCCRGX_VEL_UNIFORM=0.  The densities are
 * bitwise the same either way.  No reference counterpart. */
int dccrgx_advection_velocity_source(dccrgx_grid* g, const int fids[7], int* mask);

/* Whether the tile sweeps of fields fids divide or multiply where the divisor
 * is a power of two: *out = 1 - a face between two cells of one level
 * multiplies its velocity sum by 1 / (2 l_a) and a cell its flux sum by
 * 1 / (lx ly lz), both from the per-level table; a face between two levels
 * still divides.  That needs the table (dccrgx_advection_length_source is 1)
 * and level-0 cell lengths that are powers of two on all three axes such that
 * at each of the 32 levels the length, 2 l_a, the volume and their
 * reciprocals are normal doubles: decided on the host when the table is
 * filled, one verdict for the three axes.  0: the sweeps divide everywhere
 * (some axis fails, no table, or DCCRGX_DIV_POW2=0).  A product with an exact
 * reciprocal rounds the real number the quotient rounds, so the densities are
 * bitwise the same either way.  dccrgx_advection_layout's byte counts do not
 * depend on it.  No reference counterpart. */
int dccrgx_advection_divide_source(dccrgx_grid* g, const int fids[7], int* out);

/* ---- Poisson solver (tests/poisson/poisson_solve.hpp:156-1056) ----------
 * dccrgx_poisson_cache = Poisson_Solve::cache_system_info (827-971): local
 * cells default to boundary cells, ids in skip_cells are skipped, ids in
 * solve_cells are solved (non-local ids are ignored, as the reference does);
 * computes the geometry factors (set_scaling_factor 696-819) on the device and
 * halos them.  rhs / solution are fp64 fields.  The factors are those of the
 * geometry at this call, Cartesian or stretched, as in the reference: a later
 * dccrgx_set_geometry or dccrgx_set_stretched_geometry takes effect at the
 * next dccrgx_poisson_cache, and a solve without one (cache_is_up_to_date)
 * keeps the old factors.
 * dccrgx_poisson_solve = Poisson_Solve::solve (251-522, failsafe = 0) or
 * solve_failsafe (531-634, failsafe = 1) with the constructor's parameters
 * (187-201); solution = best solution on return.  *iterations = iterations
 * done, *residual = smallest residual (solve) or last norm (failsafe).
 * dccrgx_poisson_field: the solver's per-cell state as a field ("p0", "p1",
 * "r0", "r1", "A_dot_p0", "best_solution", "scaling_factor", "f_x_neg" ...
 * "f_z_pos", "type"), e.g. for inspection after a solve. */
int dccrgx_poisson_cache(dccrgx_grid* g, int rhs_field, int solution_field, const uint64_t* solve_cells,
                         size_t n_solve, const uint64_t* skip_cells, size_t n_skip);
int dccrgx_poisson_solve(dccrgx_grid* g, unsigned max_iterations, unsigned min_iterations, double stop_residual,
                         double p_of_norm, double stop_after_residual_increase, int failsafe, unsigned* iterations,
                         double* residual);
int dccrgx_poisson_field(dccrgx_grid* g, const char* name, int* field_id);

/* ---- collectives for user kernels (MPI_Allreduce in solve.hpp:317) ------- */
int dccrgx_allreduce_f64(dccrgx_grid* g, double* inout, int count, int op /* 0 sum, 1 min, 2 max */);
/* MPI_Allreduce on DEVICE doubles (dccrg_mpi_support.hpp All_Reduce's role
 * for fp64), queued on the compute stream: the processes' values are
 * all-gathered on the device and combined in rank order by one kernel, so
 * the result is bitwise dccrgx_allreduce_f64's and, over RCCL, nothing waits
 * on the host (a host exchange transport stages through the host).  d_in may
 * equal d_out (ABI 8) */
int dccrgx_allreduce_f64_device(dccrgx_grid* g, const double* d_in, double* d_out, int count, int op);
int dccrgx_barrier(dccrgx_grid* g);

/* The transport the grid was built on (no reference counterpart; the
 * reference's MPI_Comm_size on its duplicated communicator): *kind is
 * DCCRGX_TRANSPORT_NONE (a detached view), _RCCL or _HOST (an exchange
 * function), *comm_ranks the ranks of the communicator the library holds -
 * ncclCommCount of its RCCL communicator, the grid's size for a host exchange,
 * 1 for a detached view (ABI 9) */
#define DCCRGX_TRANSPORT_NONE 0
#define DCCRGX_TRANSPORT_RCCL 1
#define DCCRGX_TRANSPORT_HOST 2
int dccrgx_get_transport(dccrgx_grid* g, int* kind, int* comm_ranks);

/* Transport check (no reference counterpart): the bytes of a fixed-size
 * field's slots [slot0, slot0 + n) sent by this process to itself and
 * received straight into slots [dst_slot0, dst_slot0 + n) of the same field,
 * through the grid's RCCL byte mover (one grouped ncclSend / ncclRecv, the
 * path of every halo and migration message; a grid created with an RCCL id,
 * also at size 1).  Under send_single_cells the n elements go out as n
 * messages, as a halo's cells do (ABI 9).  DCCRGX_EINVAL on a host-exchange
 * or detached grid. */
int dccrgx_comm_loopback(dccrgx_grid* g, int field_id, size_t slot0, size_t n, size_t dst_slot0);

/* ---- stream / timing ----------------------------------------------------- */
int dccrgx_synchronize(dccrgx_grid* g);
void* dccrgx_compute_stream(dccrgx_grid* g);
/* average duration (ms) of the last `count` sweep kernels measured with HIP
 * events on the compute stream; enable=1 starts recording */
int dccrgx_kernel_timing(dccrgx_grid* g, int enable, double* total_ms, int64_t* count);

#ifdef __cplusplus
}
#endif

#endif /* DCCRGX_H */
