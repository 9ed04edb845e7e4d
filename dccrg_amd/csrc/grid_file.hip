// Grid files: the reader and the writer behind the dccrgx_*_grid_data entry
// points (host code only; the C ABI wrappers are in api.hip).
// save_grid_data / load_grid_data (dccrg.hpp:1089-1740, 1742-2425), file
// layout 1104-1120: `offset` bytes left alone, the caller's header, uint64
// 0x1234567890abcdef, the grid block (Mapping::write dccrg_mapping.hpp:576 =
// 3 x uint64 length + int max_ref_lvl; the neighborhood length as unsigned;
// Grid_Topology::write dccrg_topology.hpp:144 = 3 x uint8 periodic;
// Cartesian_Geometry::write dccrg_cartesian_geometry.hpp:618 = int id 1 +
// 3 x double start + 3 x double level-0 length), uint64 total cells, per
// cell (uint64 id, uint64 absolute byte offset of its data) rank by rank,
// then the cell data in the same order.  A cell's data = the payload of
// every transferred field, in field order (the reference writes what
// get_mpi_datatype describes at save time: a fixed-size field's window, a
// variable-size field's bytes of the cell).  Cells of a rank in ascending id
// (the reference: get_cells() order).  Every rank writes its own records with
// pwrite at offsets derived from the all-gathered per-rank cell counts.
#include <algorithm>
#include <cstring>
#include <numeric>
#include <unordered_map>

#include <fcntl.h>
#include <unistd.h>

#include "dccrgx_grid.hpp"

namespace dccrgx {

static constexpr uint64_t kEndianCheck = 0x1234567890abcdefULL;

static std::vector<uint8_t> grid_block(const Grid& g) {
	std::vector<uint8_t> b;
	auto put = [&b](const void* p, size_t n) {
		const uint8_t* q = static_cast<const uint8_t*>(p);
		b.insert(b.end(), q, q + n);
	};
	put(g.len, 24);
	const int32_t R = g.R;
	put(&R, 4);
	const uint32_t hood = g.hood_len;
	put(&hood, 4);
	const uint8_t per[3] = {uint8_t(g.per[0] != 0), uint8_t(g.per[1] != 0), uint8_t(g.per[2] != 0)};
	put(per, 3);
	if (!g.geo_block.empty()) {
		put(g.geo_block.data(), g.geo_block.size());  // the stretched geometry's block
		return b;
	}
	const int32_t gid = kCartesianGeometryId;
	put(&gid, 4);
	put(g.start, 24);
	put(g.l0, 24);
	return b;
}

static void pwrite_all(int fd, const void* p, size_t n, uint64_t off) {
	const uint8_t* q = static_cast<const uint8_t*>(p);
	while (n) {
		const ssize_t w = ::pwrite(fd, q, n, off_t(off));
		DX_REQUIRE(w > 0, "grid file write failed");
		q += w;
		n -= size_t(w);
		off += uint64_t(w);
	}
}

static void pread_all(int fd, void* p, size_t n, uint64_t off) {
	uint8_t* q = static_cast<uint8_t*>(p);
	while (n) {
		const ssize_t r = ::pread(fd, q, n, off_t(off));
		DX_REQUIRE(r > 0, "grid file truncated");
		q += r;
		n -= size_t(r);
		off += uint64_t(r);
	}
}

struct Closer {
	int fd;
	~Closer() { ::close(fd); }
};

// The bytes a field adds to one cell's record: a fixed-size field the window
// its get_mpi_datatype describes (the whole element by default), a
// variable-size field the cell's own bytes (save_grid_data writes what each
// cell's datatype describes, 1521-1540; padding is not written, 1529).
void save_grid_impl(Grid& g, const char* path, uint64_t offset, const void* header, size_t header_bytes) {
	DX_REQUIRE(g.initialized, "not initialized");
	const std::vector<Field*> tf = transfer_fields(g);
	const size_t nl = g.n_local;
	// the local slots' payloads on the host, and each cell's record length
	std::vector<std::vector<uint8_t>> host(tf.size());
	std::vector<std::vector<uint64_t>> voff(tf.size());
	std::vector<uint64_t> rec(nl, 0);
	for (size_t k = 0; k < tf.size(); k++) {
		const Field* f = tf[k];
		if (f->var) {
			voff[k] = download(f->voff.p, nl + 1, g.s_comp);
			host[k] = download(f->data.p + voff[k][0], voff[k][nl] - voff[k][0], g.s_comp);
			for (size_t s = 0; s < nl; s++) rec[s] += voff[k][s + 1] - voff[k][s];
		} else {
			host[k] = download(f->data.p, nl * f->elem, g.s_comp);
			for (size_t s = 0; s < nl; s++) rec[s] += f->win_len;
		}
	}
	const uint64_t mine = std::accumulate(rec.begin(), rec.end(), uint64_t(0));
	const auto cnt = comm_allgather_u64(g, {uint64_t(nl), mine});
	uint64_t total = 0, before = 0, bytes_before = 0, bytes_total = 0;
	for (int p = 0; p < g.size; p++) {
		const auto& c = cnt[size_t(p)];
		DX_REQUIRE(c.size() == 2, "grid file: inconsistent cell counts");
		if (p < g.rank) {
			before += c[0];
			bytes_before += c[1];
		}
		total += c[0];
		bytes_total += c[1];
	}
	const int fd = ::open(path, O_CREAT | O_WRONLY, 0644);
	DX_REQUIRE(fd >= 0, std::string("cannot open grid file ") + path);
	Closer closer{fd};
	uint64_t off = offset;
	if (g.rank == 0 && header_bytes) pwrite_all(fd, header, header_bytes, off);
	off += header_bytes;
	if (g.rank == 0) pwrite_all(fd, &kEndianCheck, 8, off);
	off += 8;
	const std::vector<uint8_t> block = grid_block(g);
	if (g.rank == 0) pwrite_all(fd, block.data(), block.size(), off);
	off += block.size();
	if (g.rank == 0) pwrite_all(fd, &total, 8, off);
	off += 8;
	const uint64_t list0 = off, data0 = off + 16 * total + bytes_before;
	// local cells ascending, with their slots
	const auto& sid = slot_ids_host(g);
	std::vector<uint32_t> order(nl);
	std::iota(order.begin(), order.end(), 0u);
	std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return sid[a] < sid[b]; });
	std::vector<uint64_t> list(2 * nl);
	std::vector<uint8_t> data(mine);
	uint64_t at = 0;
	for (size_t i = 0; i < nl; i++) {
		const size_t s = order[i];
		list[2 * i] = sid[s];
		list[2 * i + 1] = data0 + at;
		for (size_t k = 0; k < tf.size(); k++) {
			const Field* f = tf[k];
			if (f->var) {
				const uint64_t a = voff[k][s] - voff[k][0], n = voff[k][s + 1] - voff[k][s];
				if (n) std::memcpy(&data[at], &host[k][a], n);
				at += n;
			} else {
				if (f->win_len) std::memcpy(&data[at], &host[k][s * f->elem + f->win_off], f->win_len);
				at += f->win_len;
			}
		}
	}
	if (nl) pwrite_all(fd, list.data(), 16 * nl, list0 + 16 * before);
	if (mine) pwrite_all(fd, data.data(), data.size(), data0);
	// Like the reference (MPI_MODE_CREATE | MPI_MODE_WRONLY, dccrg.hpp:1131)
	// bytes already in the file past the grid data stay - except
	// when a variable-size field is saved: the one-shot load_grid_data takes
	// such a field's bytes up to the record's end, and the last record ends at
	// the end of the file, so stale bytes of an older, longer file there would
	// become the last cell's payload.  Then rank 0 cuts the file at
	// the end of the grid data (every rank's records lie before it).
	const uint64_t data_end = list0 + 16 * total + bytes_total;
	if (g.rank == 0 && !var_transfer_fields(g).empty()) {
		const off_t cur = ::lseek(fd, 0, SEEK_END);
		DX_REQUIRE(cur >= 0, "grid file size unknown");
		if (uint64_t(cur) > data_end) DX_REQUIRE(::ftruncate(fd, off_t(data_end)) == 0, "grid file: truncate failed");
	}
}

// start_loading_grid_data (1795-2083): the grid block and the cell list; every
// local cell's record position, none of its payload
void start_load_impl(Grid& g, const char* path, uint64_t offset, size_t header_bytes) {
	DX_REQUIRE(!g.initialized, "load_grid_data initializes the grid: call it instead of initialize");
	const int fd = ::open(path, O_RDONLY);
	DX_REQUIRE(fd >= 0, std::string("cannot open grid file ") + path);
	Closer closer{fd};
	const off_t file_end = ::lseek(fd, 0, SEEK_END);
	DX_REQUIRE(file_end >= 0, "grid file size unknown");
	uint64_t off = offset + header_bytes, endian = 0;
	pread_all(fd, &endian, 8, off);
	DX_REQUIRE(endian == kEndianCheck, "grid file endianness check failed");
	off += 8;
	// mapping + neighborhood length + topology (35 B), then the geometry block:
	// Cartesian (id 1, 52 B) or stretched (id 2, 28 B + the coordinates)
	uint8_t blk[87];
	static_assert(35 + kStretchedBlockHead <= sizeof(blk), "the stretched block's head is read with the grid block");
	pread_all(fd, blk, 35 + kStretchedBlockHead, off);
	uint64_t len[3];
	int32_t R, gid;
	uint32_t hood;
	double start[3], l0[3];
	std::memcpy(len, blk, 24);
	std::memcpy(&R, blk + 24, 4);
	std::memcpy(&hood, blk + 28, 4);
	std::memcpy(&gid, blk + 35, 4);
	std::vector<uint8_t> geo;
	if (gid == kStretchedGeometryId) {
		const size_t nb = stretched_block_bytes(blk + 35);
		DX_REQUIRE(nb > 0 && nb <= uint64_t(file_end) - (off + 35), "grid file: invalid stretched geometry block");
		geo.resize(nb);
		pread_all(fd, geo.data(), nb, off + 35);
		std::vector<double> c[3];
		stretched_block_coords(geo, c);
		// the library's device geometry: each dimension's start and first
		// level-0 cell length (exact for evenly spaced coordinates; uneven
		// spacing stays with the facade's host-side geometry)
		for (int d = 0; d < 3; d++) {
			start[d] = c[d][0];
			l0[d] = c[d][1] - c[d][0];
		}
		off += 35 + nb;
	} else {
		DX_REQUIRE(gid == kCartesianGeometryId,
		           "grid file geometry is neither Cartesian_Geometry nor Stretched_Cartesian_Geometry");
		pread_all(fd, blk + 63, 24, off + 63);
		std::memcpy(start, blk + 39, 24);
		std::memcpy(l0, blk + 63, 24);
		off += sizeof(blk);
	}
	// the same checks as the setters (a foreign or corrupt file must not
	// reach the builders)
	for (int d = 0; d < 3; d++) DX_REQUIRE(len[d] > 0, "grid file: grid length must be > 0");
	DX_REQUIRE(R >= 0 && R <= max_possible_level(len) && R < kMaxLevels, "grid file: invalid refinement level");
	DX_REQUIRE(hood <= max_hood_length(), "grid file: neighborhood length not supported");
	for (int d = 0; d < 3; d++) DX_REQUIRE(l0[d] > 0, "grid file: cell length must be > 0");
	for (int d = 0; d < 3; d++) {
		g.len[d] = len[d];
		g.per[d] = blk[32 + d] != 0;
		g.start[d] = start[d];
		g.l0[d] = l0[d];
	}
	g.R = R;
	g.hood_len = hood;
	g.geo_block = std::move(geo);
	g.str.drop();
	init_impl(g);
	uint64_t total = 0;
	pread_all(fd, &total, 8, off);
	off += 8;
	DX_REQUIRE(total <= (uint64_t(file_end) - off) / 16, "grid file truncated");
	std::vector<uint64_t> list(2 * total);
	if (total) pread_all(fd, list.data(), 16 * total, off);
	const uint64_t data_start = off + 16 * total;
	// a record ends where the next one starts, the last at the end of the
	// file: in list order when the offsets never decrease along the list (the
	// files save_grid_data writes, rank by rank, each rank's cells in the
	// order of their data; empty records then stay empty), else in the order
	// of the offsets
	bool monotone = true;
	for (size_t i = 0; i < total; i++) {
		const uint64_t p = list[2 * i + 1];
		DX_REQUIRE(p >= data_start && p <= uint64_t(file_end), "grid file: cell data out of range");
		if (i && p < list[2 * i - 1]) monotone = false;
	}
	std::vector<uint64_t> starts(total);
	for (size_t i = 0; i < total; i++) starts[i] = list[2 * i + 1];
	std::sort(starts.begin(), starts.end());
	struct Rec {
		uint64_t id, pos, end;
		bool operator<(const Rec& o) const { return id < o.id; }
	};
	std::vector<Rec> cells(total);
	for (size_t i = 0; i < total; i++) {
		const uint64_t p = list[2 * i + 1];
		uint64_t e = uint64_t(file_end);
		if (monotone) {
			if (i + 1 < total) e = list[2 * i + 3];
		} else {
			auto nx = std::upper_bound(starts.begin(), starts.end(), p);
			if (nx != starts.end()) e = *nx;
		}
		cells[i] = {list[2 * i], p, e};
	}
	if (!monotone) {
		// records sharing a start: only the last of them in list order holds
		// bytes, the others are empty (as a writer lays out an empty record
		// followed by a full one at the same position)
		std::unordered_map<uint64_t, size_t> last;
		for (size_t i = 0; i < total; i++) last[list[2 * i + 1]] = i;
		for (size_t i = 0; i < total; i++)
			if (last[list[2 * i + 1]] != i) cells[i].end = cells[i].pos;
	}
	std::sort(cells.begin(), cells.end());
	// owners as load_cells (3647) produces them: the level-0 block
	// partition (create_level_0_cells), refined cells inherit it
	std::vector<uint64_t> ids(total);
	std::vector<int32_t> own(total);
	for (size_t i = 0; i < total; i++) {
		ids[i] = cells[i].id;
		DX_REQUIRE(i == 0 || ids[i] > ids[i - 1], "grid file lists a cell twice");
		const uint64_t l0p = map_level0_parent(g.m, ids[i]);
		DX_REQUIRE(l0p != error_cell, "grid file lists an invalid cell");
		own[i] = g.mesh.bp.owner(l0p);
	}
	Mesh nm;
	mesh_from_global(g, nm, ids, own);
	rebuild(g, nm);
	const size_t nl = g.n_local;
	const auto& sid = slot_ids_host(g);
	g.load.pos.assign(nl, 0);
	g.load.end.assign(nl, 0);
	for (size_t i = 0; i < nl; i++) {
		auto it = std::lower_bound(cells.begin(), cells.end(), Rec{sid[i], 0, 0});
		DX_REQUIRE(it != cells.end() && it->id == sid[i], "local cell missing from grid file");
		g.load.pos[i] = it->pos;
		g.load.end[i] = it->end;
	}
	g.load.path = path;
	g.load.active = true;
}

// continue_loading_grid_data (2112-2378): the next bytes of every local
// cell's record into one field, from the cell's position on, which then
// advances past them.  bytes[s]: the count for local slot s (a fixed-size
// field: its window).  Reads coalesce records that lie close together.
void continue_load_impl(Grid& g, int fid, const uint64_t* sizes) {
	DX_REQUIRE(g.load.active, "no grid file being loaded (start_loading_grid_data first)");
	Field& f = field(g, fid);
	const size_t nl = g.n_local;
	DX_REQUIRE(g.load.pos.size() == nl, "the grid changed while loading a grid file");
	DX_REQUIRE(!f.var || sizes || !nl, "a variable-size field needs the byte count of every local cell");
	std::vector<uint64_t> bytes(nl);
	for (size_t s = 0; s < nl; s++) {
		bytes[s] = f.var ? sizes[s] : f.win_len;
		DX_REQUIRE(bytes[s] <= g.load.end[s] - g.load.pos[s],
		           "grid file: cell " + std::to_string(slot_ids_host(g)[s]) + " has fewer bytes left than requested");
	}
	const int fd = ::open(g.load.path.c_str(), O_RDONLY);
	DX_REQUIRE(fd >= 0, "cannot open grid file " + g.load.path);
	Closer closer{fd};
	// slot order -> file order, then runs with gaps under 64 KiB read at once
	std::vector<uint32_t> by_pos(nl);
	std::iota(by_pos.begin(), by_pos.end(), 0u);
	std::sort(by_pos.begin(), by_pos.end(), [&](uint32_t a, uint32_t b) { return g.load.pos[a] < g.load.pos[b]; });
	std::vector<uint64_t> at(nl + 1, 0);  // the slot's bytes in `got` (slot order)
	for (size_t s = 0; s < nl; s++) at[s + 1] = at[s] + bytes[s];
	std::vector<uint8_t> got(at[nl]);
	std::vector<uint8_t> run;
	for (size_t i = 0; i < nl;) {
		const uint64_t lo = g.load.pos[by_pos[i]];
		uint64_t hi = lo + bytes[by_pos[i]];
		size_t j = i + 1;
		while (j < nl && g.load.pos[by_pos[j]] <= hi + 65536 && g.load.pos[by_pos[j]] - lo < (uint64_t(1) << 30)) {
			hi = std::max(hi, g.load.pos[by_pos[j]] + bytes[by_pos[j]]);
			j++;
		}
		if (hi > lo) {
			run.resize(hi - lo);
			pread_all(fd, run.data(), run.size(), lo);
			for (size_t k = i; k < j; k++) {
				const uint32_t s = by_pos[k];
				if (bytes[s]) std::memcpy(&got[at[s]], &run[g.load.pos[s] - lo], bytes[s]);
			}
		}
		i = j;
	}
	if (f.var) {
		DBuf<uint64_t> all;
		all.alloc(g.n_slots + 1);
		var_sizes(f, nullptr, 0, g.n_slots, all.p, g.s_comp);
		if (nl) h2d(all.p, bytes.data(), nl * 8, g.s_comp);
		var_resize(f, g.n_slots, all.p, g.s_comp);
		if (at[nl]) {
			HIP_CHECK(hipMemcpyAsync(f.data.p, got.data(), got.size(), hipMemcpyHostToDevice, g.s_comp));
			HIP_CHECK(hipStreamSynchronize(g.s_comp));
		}
	} else if (nl && f.win_len) {
		// the window of every element; the rest of it keeps its bytes
		std::vector<uint8_t> h = download(f.data.p, nl * f.elem, g.s_comp);
		for (size_t s = 0; s < nl; s++) std::memcpy(&h[s * f.elem + f.win_off], &got[at[s]], f.win_len);
		{
			HIP_CHECK(hipMemcpyAsync(f.data.p, h.data(), h.size(), hipMemcpyHostToDevice, g.s_comp));
			HIP_CHECK(hipStreamSynchronize(g.s_comp));
		}
	}
	for (size_t s = 0; s < nl; s++) g.load.pos[s] += bytes[s];
	field_written(f);
}

// finish_loading_grid_data (2380-2400)
void finish_load_impl(Grid& g) {
	DX_REQUIRE(g.load.active, "no grid file being loaded");
	g.load = Grid::FileLoad{};
}

// what is left of every local cell's record, for the caller's byte counts
void grid_file_bytes_left(Grid& g, uint64_t* bytes) {
	DX_REQUIRE(g.load.active, "no grid file being loaded");
	DX_REQUIRE(bytes || !g.n_local, "null pointer");
	for (size_t s = 0; s < g.n_local; s++) bytes[s] = g.load.end[s] - g.load.pos[s];
}

// load_grid_data (1742-1790) = start, one continue over the transferred
// fields in field order, finish.  A variable-size field takes what is left of
// each record after the fixed-size fields that follow it, so at most one
// variable-size field can be read this way (more need the split load with
// the caller's byte counts, as the reference's multi-pass example
// tests/restart/variable_cell_data.cpp does).
void load_grid_impl(Grid& g, const char* path, uint64_t offset, size_t header_bytes) {
	DX_REQUIRE(var_transfer_fields(g).size() <= 1,
	           "several variable-size fields: load with start / continue / finish_loading_grid_data");
	start_load_impl(g, path, offset, header_bytes);
	const std::vector<Field*> tf = transfer_fields(g);
	for (size_t k = 0; k < tf.size(); k++) {
		Field* f = tf[k];
		if (!f->var) {
			continue_load_impl(g, int(f - g.fields.data()), nullptr);
			continue;
		}
		uint64_t after = 0;
		for (size_t j = k + 1; j < tf.size(); j++) after += tf[j]->win_len;
		std::vector<uint64_t> sz(g.n_local);
		for (size_t s = 0; s < g.n_local; s++) {
			const uint64_t left = g.load.end[s] - g.load.pos[s];
			DX_REQUIRE(left >= after, "grid file: a cell's record is shorter than its fixed-size fields");
			sz[s] = left - after;
		}
		continue_load_impl(g, int(f - g.fields.data()), sz.data());
	}
	finish_load_impl(g);
}

}  // namespace dccrgx
