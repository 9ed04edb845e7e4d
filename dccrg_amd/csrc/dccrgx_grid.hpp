// Host driver functions: what api.hip (the C ABI) calls and what the drivers'
// files (grid.hip, mesh.hip, advection.hip, particles.hip, poisson.hip, ...)
// share.
#pragma once

#include "dccrgx_internal.hpp"

namespace dccrgx {

std::vector<Field*> transfer_fields(Grid& g);
Field& field(Grid& g, int fid);
Field& fixed_field(Grid& g, int fid);  // EINVAL for a variable-size field
std::vector<Field*> var_transfer_fields(Grid& g);
void ensure_scratch(Grid& g, Field& f);
void commit(Grid& g, Field& f);
void region_range(const Grid& g, int region, size_t& s0, size_t& s1);
void drain_timing(Grid& g);

void halo_start(Grid& g);
void halo_wait(Grid& g);
UserHood& ensure_uhood(Grid& g, int id);
HaloPlan& plan_of(Grid& g, int hood);
void uhood_halo(Grid& g, int id);
size_t halo_pack_peer(Grid& g, int hood, int peer, uint8_t* buf, size_t cap);
void halo_place_peer(Grid& g, int hood, int peer, const uint8_t* buf, size_t bytes);
void halo_message_size(Grid& g, int hood, int peer, size_t& sb, size_t& rb);

void stop_refining_impl(Grid& g);  // the created cells in Grid::new_cells
// the requests stop_refining takes: the status the ABI returns (ENOTFOUND by
// value for a refused cell, so dccrgx_last_error stays as it was);
// flush_bulk_requests merges the bulk request lists into the sets first
void flush_bulk_requests(Grid& g);
int refine_completely(Grid& g, uint64_t cell);
int unrefine_completely(Grid& g, uint64_t cell);

void initialize_balance_load_impl(Grid& g, bool use_partitioner, const uint64_t* cells, const int32_t* procs,
                                  size_t n);
// partition.hip: recursive coordinate bisection of the leaves (the new
// owner of every local cell, cells ascending); collective
void rcb_partition(Grid& g, std::vector<uint64_t>& cells, std::vector<int32_t>& owners);
void continue_balance_load_impl(Grid& g);
void finish_balance_load_impl(Grid& g);
void migration_message_size(Grid& g, int peer, size_t& sb, size_t& rb);
void migration_pack_peer(Grid& g, int peer, uint8_t* buf, size_t cap);
void migration_place_peer(Grid& g, int peer, const uint8_t* buf, size_t bytes);

std::vector<uint64_t> cells_by_criteria(Grid& g, const int32_t* crit, size_t nc, bool exact, int hood);
int64_t host_slot_of(Grid& g, uint64_t id);
// grid.hip: what the setters, dccrgx_initialize and the grid-file loader
// share: the limits of the refinement level and of the neighborhood length,
// and the first build of the mesh
int max_possible_level(const uint64_t len[3]);
unsigned max_hood_length();
void init_impl(Grid& g);
// gol.hip: dccrgx_gol_step, one step of the uniform game of life into the
// state field's scratch (kernels and driver)
void gol_step(Grid& g, int sf, int region);
// gol_amr.hip: the refined game of life, one phase (0 collect, 1 spread) over
// a region or a whole turn with its halo; the reference's aborts are raised
void gol_amr_phase(Grid& g, int phase, int sf, int lf, int region);
void gol_live_neighbors(Grid& g, int sf, int lf);
// mesh.hip: dccrgx_mapping_batch, the device id math for n host ids (level[i]
// and 15 words per id)
void mapping_batch(Grid& g, const uint64_t* ids, size_t n, int32_t* level, uint64_t* out);

// poisson.hip: the Poisson solver's driver, one function per dccrgx_poisson_*
// entry point of dccrgx.h (the kernels: poisson_kernels.hip)
void poisson_cache(Grid& g, int rhs, int sol, const uint64_t* solve, size_t ns, const uint64_t* skip, size_t nk);
void poisson_solve(Grid& g, unsigned max_iterations, unsigned min_iterations, double stop_residual, double p_of_norm,
                   double stop_after_residual_increase, bool failsafe, unsigned* iterations, double* residual);
int poisson_field(Grid& g, const char* name);  // the id of the solver's field "poisson.<name>"

// grid_file.hip: save_grid_data and load_grid_data, whole or in its three
// steps (sizes: a variable-size field's byte count of every local cell)
void save_grid_impl(Grid& g, const char* path, uint64_t offset, const void* header, size_t header_bytes);
void load_grid_impl(Grid& g, const char* path, uint64_t offset, size_t header_bytes);
void start_load_impl(Grid& g, const char* path, uint64_t offset, size_t header_bytes);
void continue_load_impl(Grid& g, int fid, const uint64_t* sizes);
void finish_load_impl(Grid& g);
void grid_file_bytes_left(Grid& g, uint64_t* bytes);

// field_ops.hip: the operators on fp64 cell fields, one function per entry
// point (dccrgx_gradient, _curl, _divergence, _field_axpy,
// _field_reduce_device); every check precedes the first write
void field_gradient(Grid& g, int in_field, const int out_fields[3], double scale, int region);
void field_curl(Grid& g, const int in_fields[3], const int out_fields[3], double scale, bool accumulate, int region);
void field_divergence(Grid& g, const int in_fields[3], int out_field, double scale, bool accumulate, int region);
void field_axpy(Grid& g, int y_field, double a, int x_field, int region);
void field_reduce_device(Grid& g, const int* terms, int n, int by_volume, int region, int collective, double* d_out);

// advection.hip: the advection solver's driver, one function per
// dccrgx_advection_* entry point of dccrgx.h (fids: rho vx vy vz lx ly lz)
void advection_step(Grid& g, const int fids[7], double dt, int region);
void advection_layout(Grid& g, uint64_t out[12]);
void advection_occupancy(Grid& g, uint64_t out[6]);
void advection_length_source(Grid& g, const int fids[7], int* out);
void advection_velocity_source(Grid& g, const int fids[7], int* mask);
void advection_divide_source(Grid& g, const int fids[7], int* out);
void advection_commit(Grid& g, int df);
void advection_initialize(Grid& g, const int fids[7]);
void advection_max_time_step(Grid& g, const int fids[7], double* out);
void advection_max_time_step_device(Grid& g, const int fids[7], double* d_out);
std::vector<uint64_t> advection_refine_candidates(Grid& g, int df, double diff_increase, double diff_threshold);
void advection_check_adaptation(Grid& g, int df, double diff_increase, double diff_threshold,
                                double unrefine_sensitivity, uint64_t counts[3]);
void advection_adapt(Grid& g, const int fids[7], uint64_t out[2]);

// particles.hip: the smallest known leaf at each of n host coordinates
// (error_cell: none), and one push / locate / re-bin step of a variable field
// of K-double particle records (stats: stayed, moved, arrived, handed over, lost)
void existing_cells_at(Grid& g, const double* xyz, size_t n, uint64_t* ids);
void particles_step(Grid& g, int fid, int K, const double* velocity, double dt, uint64_t stats[5]);
// particles follow the mesh through stop_refining (Field::follow_K records):
// follow_set turns it on (K >= 3) or off (K == 0); follow_check, before the
// mesh changes, is false when a local cell's bytes are no whole records;
// follow_rebuild replaces var_remap in stop_refining's rebuild: the records
// of a refined old local cell go to the children point location names on the
// new mesh, a merged family's parent takes the removed store's records
void particles_follow_set(Grid& g, int fid, int K);
bool particles_follow_check(Grid& g, const Field& f);
void particles_follow_rebuild(Grid& g, Field& f, const uint64_t* old_ids, size_t n_old_local, const DevMesh& newM,
                              size_t new_n_slots, size_t new_n_local, hipStream_t s);
// cell fields follow the mesh through stop_refining (Field::follow_mode,
// field_adapt.hip): follow_set checks and stores the mode; slope_pass, with
// the refine set final and the old mesh still standing, leaves Grid::fslopes
// for the LINEAR fields (nothing when there is none or nothing is refined);
// follow_restrict, after the rebuild, gives the merged parents of the fields
// `fids` their children's mean or sum from the removed store
void field_follow_set(Grid& g, int fid, int mode);
void field_slope_pass(Grid& g, const uint64_t* refined_dev, size_t n_refined);
void field_follow_restrict(Grid& g, const std::vector<int>& fids);
// particles <-> cell fields with the weight W(p, c) of dccrgx.h (shape 0 NGP,
// 1 CIC over leaves): deposit sums q W over the records of a local cell and
// of the distinct leaves of its neighbors_of into a fixed fp64 field; gather
// writes sum W F_j[c] of n fixed fp64 fields into doubles first_double .. of
// every record of a local cell
void particles_deposit(Grid& g, int fid, int K, int shape, int weight_double, int out_fid, int per_volume);
void particles_gather(Grid& g, int fid, int K, int shape, const int* cell_fields, int n, int first_double);
// record[3 + j] += (factor q) record[first_double + j], j < 3, for every
// record of a local cell (q = record[weight_double], or 1 with -1)
void particles_accelerate(Grid& g, int fid, int K, int first_double, int weight_double, double factor);
// n moments (q * record[factors[2 j]]) * record[factors[2 j + 1]] (-1: 1.0) of
// the records in the deposit's walk, W formed once per (record, receiver);
// factors (-1, -1) give the deposit's bits
void particles_deposit_moments(Grid& g, int fid, int K, int shape, int weight_double, const int* factors,
                               const int* out_fids, int n, int per_volume);
// the Boris kick of dccrgx.h with E at e_first .., B at b_first ..,
// h = factor q, for every record of a local cell
void particles_boris(Grid& g, int fid, int K, int e_first, int b_first, int weight_double, double factor);
// dccrgx_particles_create: n_c new records behind every local cell's own,
// every value a function of (seed, cell id, index, double); *created: their
// number on this process
void particles_create(Grid& g, int fid, int K, int count_field, double count, int round_random, const int* recipe_i,
                      const double* recipe_d, uint64_t seed, uint64_t* created);
// dccrgx_particles_remove: the records of the local cells that a mask, a test
// or chance removes leave their lists (a stable compaction per cell), their
// moments are tallied per cell and they may be appended to into_fid's lists;
// stats: kept, removed by mask, by a test, by chance
void particles_remove(Grid& g, int fid, int K, const int* test_i, const double* test_d, int n_tests, int mask_fid,
                      int prob_fid, double prob, uint64_t seed, int rescale, int weight_double,
                      const int* tally_factors, const int* tally_fids, int n_tally, int into_fid, uint64_t stats[4]);
// n reductions terms[3 j] (DCCRGX_REDUCE_*) over (q * record[terms[3 j + 1]]) *
// record[terms[3 j + 2]] (-1: 1.0) of the local cells' records into the device
// doubles d_out, queued on the compute stream; collective: combined over the
// processes in rank order
void particles_reduce(Grid& g, int fid, int K, int weight_double, const int* terms, int n, int collective,
                      double* d_out);
// the source of V_c for dccrgx_field_reduce's by_volume (the deposit's
// per_volume rule and cell_volume's bits)
RedVolume reduce_volume(Grid& g, bool by_volume);
// the active stretched geometry's coordinates on the device (x, then y, then
// z, packed), uploaded at first use
const double* stretched_device(Grid& g);
// the same with each dimension's offset, for the Poisson cache pass and the
// advection reset pass (Cartesian grid: c == nullptr, nothing uploaded)
StretchedView stretched_view(Grid& g);
// the stencil arguments of the kernels over the face table, the table built
inline FaceStencil face_stencil(Grid& g) {
	ensure_face(g);
	return {g.m, g.l0, stretched_view(g), g.slot_ids.p, g.slot_lvl.p, g.face_ell.p, g.face_fine.p};
}
// geometry.hip: the fp64 center and / or length of every slot's cell into
// fixed-size fp64 fields (-1: none), Cartesian or stretched
void geometry_fill(Grid& g, const int center_fields[3], const int length_fields[3]);
// the same on the host for n ids (NaN for an id that is no cell)
void geometry_batch(Grid& g, const uint64_t* ids, size_t n, double* center, double* length);
// the stretched geometry from three coordinate arrays (checked), and a
// geometry block for the grid file alone (n == 0: none)
void set_stretched_geometry(Grid& g, const double* const coords[3], const size_t n[3]);
void set_geometry_block(Grid& g, const void* bytes, size_t n);
// the geometry block of a grid file (after mapping, neighborhood length and
// topology): its first int names the geometry.  The stretched one's block is
// kStretchedBlockHead bytes (the id, three uint64 coordinate counts) and the
// coordinates: stretched_block builds it, stretched_block_bytes sizes it from
// its head (0: no valid block), stretched_block_coords reads a checked one back
constexpr int kCartesianGeometryId = 1, kStretchedGeometryId = 2;
constexpr size_t kStretchedBlockHead = 28;
std::vector<uint8_t> stretched_block(const double* const coords[3], const size_t n[3]);
size_t stretched_block_bytes(const uint8_t* head);
void stretched_block_coords(const std::vector<uint8_t>& block, std::vector<double> c[3]);

}  // namespace dccrgx
