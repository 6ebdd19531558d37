// ldpc_bs_host.h — the host-side planning and launch helpers of ldpc_bs.hip that the compressed
// kernel's host code (ldpc_bsc.hip) uses too.
#pragma once
#include <vector>

#include "ldpc_awgn.h"
#include "ldpc_bs_kernel.h"

namespace ldpc {
namespace bs {

// the QMS grids both kernels decode
bool bs_mode(int mode);
float bs_step(int mode);
int bs_qmax(int mode);
// slot layout, lane maps, chunk dealing and the per-column rotation
std::vector<int32_t> slot_layout(const host::GraphTables& h, int LPC, size_t* nslot);
std::vector<int32_t> slot_layout_rows(const host::GraphTables& h, const std::vector<int>& rl, size_t* nslot);
std::vector<int32_t> uniform_lanes(const host::GraphTables& h, int LPC, int cn_lanes);
std::vector<int> check_chunk_cost_lanes(const host::GraphTables& h, const std::vector<int32_t>& lanes);
std::vector<int> check_chunk_cost(const host::GraphTables& h, int LPC, int cch);
std::vector<int> column_rotation_lanes(const host::GraphTables& h, int EPL, const std::vector<int32_t>& lanes);
std::vector<int> column_rotation(const host::GraphTables& h, int LPC, int EPL, int cn_lanes);
std::vector<int> deal_chunks(const std::vector<int>& cost, int nw, int cap);
void bs_stagger(bool one_per_cu, int* stagger, int* stagger_n);
// the per-decode weight tables (k_bs_tables)
int bs_make_tables(const Bufs& b, const DevGraph& g, int arows, int ar, int bcols, float step, int qmax,
                   float cu, bool ucn, FusedWorkspace& ws, uint32_t** alut, uint32_t** blut, hipStream_t s);

// the in-prologue channel of a decode (b.q8 / b.gen8; ldpc_decode_awgn) as the kernels take it, its
// tables copied to LDS byte `lds`; all zero without one
inline BsGen bs_gen(const Bufs& b, uint32_t lds) {
    BsGen gen{};
    if (!b.q8) return gen;
    const AwgnParams& g8 = *reinterpret_cast<const AwgnParams*>(b.gen8);
    gen.tab = b.q8;
    gen.k0 = g8.k0;
    gen.k1 = g8.k1;
    gen.offset = g8.offset;
    gen.nb = g8.nb;
    gen.kmin = g8.kmin;
    gen.ps = g8.ps;
    gen.pe = g8.pe;
    gen.ss = g8.ss;
    gen.se = g8.se;
    gen.lds = lds;
    return gen;
}

}  // namespace bs
}  // namespace ldpc
