// rfx_exr_import.hip — the C ABI's streamed EXR frames and EXR blocks (include/rfx.h): the file's chunks or tiles cross PCIe packed; K9
// (k9_exr_import.hip) turns them into the staged planes of rfx_stage_aov's plan (rfx_stage.hip), and the same pack launches follow.  One plan serves
// every entry point: a block is a rectangle of the frame, a scanline chunk the block with x = 0, cols = W.  The planner is a pure function of the
// descriptor and the geometry (ExrGeom): no context, no HIP call.
#include <algorithm>
#include <string>
#include <utility>
#include <vector>
#include "rfx_host.h"

struct ExrPlan {
    rfx_aov_plan aov;
    int type[RFX_AOV_PLANES], channels[RFX_AOV_PLANES];
    std::vector<K9Part> parts;
    std::vector<K9Chan> chans;
    std::vector<char> mapped;     // per part: one of its channels feeds a plane
    std::vector<K9Chunk> chunks;  // the ones the band needs, in the descriptor's order
    std::vector<unsigned long long> file_offset;  // of each of them
    unsigned long long copy_bytes = 0, packed_bytes = 0, scratch_bytes = 0;  // host -> device; the two device areas (256-byte-aligned pieces)
    int rle_chunks = 0, piz_chunks = 0;
};
// all the planner reads of a context: the frame, and the rows RFX_TEX_GBUFFER holds (VELOCITY and DIRECT_LIGHT hold the same)
// ... and the kinds of its AOV conventions (include/rfx.h): a position plane has three components, CAMERAS no velocity plane
struct ExrGeom { int W, H, held_row0, held_rows, depth_kind, velocity_kind; };
static ExrGeom exr_geom(const rfx_ctx *c) { return {c->W, c->H, c->slots[RFX_TEX_GBUFFER].row0, c->slots[RFX_TEX_GBUFFER].rows, aov_depth_kind(c), aov_velocity_kind(c)}; }
static unsigned long long align256(unsigned long long n) { return (n + 255ull) & ~255ull; }

// The parts, their channels and the planes they make.  allowed: bit k set = compression k is taken.  0, or the RFX_EINVAL case in words.
static const char *exr_parts_plan(const ExrGeom &g, const rfx_exr_part *part, int nparts, unsigned int allowed, const char *bad_compression, int row0, int rows,
                                  ExrPlan *p) {
    const int want_max[RFX_AOV_PLANES] = {4, 3, 1, 1, 3, 2, g.depth_kind == RFX_AOV_DEPTH_POSITION ? 3 : 1, 4};
    unsigned int comp_mask[RFX_AOV_PLANES] = {0}, any_float[RFX_AOV_PLANES] = {0};
    p->mapped.assign((size_t)nparts, 0);
    for (int k = 0; k < nparts; k++) {
        const rfx_exr_part &q = part[k];
        if (q.compression < 0 || q.compression > 31 || !(allowed >> q.compression & 1u)) return bad_compression;
        if (q.channels <= 0 || q.channels > 1024 || !q.channel) return "a part's channel list";
        K9Part kp = {(int)p->chans.size(), q.channels, 0u, 0u, q.compression};
        for (int i = 0; i < q.channels; i++) {
            const rfx_exr_channel &ch = q.channel[i];
            if (ch.pixel_type != RFX_EXR_HALF && ch.pixel_type != RFX_EXR_FLOAT) return "a channel's pixel type must be HALF or FLOAT (UINT channels are not streamed)";
            if (ch.plane < RFX_EXR_SKIP || ch.plane >= RFX_AOV_PLANES) return "a channel's plane";
            const bool half = ch.pixel_type == RFX_EXR_HALF;
            if (ch.plane >= 0) {
                if (ch.component < 0 || ch.component >= want_max[ch.plane]) return "a channel's component";
                if (comp_mask[ch.plane] & (1u << ch.component)) return "two channels feed one component of a plane";
                comp_mask[ch.plane] |= 1u << ch.component;
                any_float[ch.plane] |= half ? 0u : 1u;
                p->mapped[k] = 1;
            }
            p->chans.push_back({half ? 1 : 0, ch.plane, ch.plane >= 0 ? ch.component : 0, kp.texel_bytes, kp.pxr_bytes});
            kp.texel_bytes += half ? 2u : 4u;  // (at most 1024 channels: <= 4096)
            kp.pxr_bytes += half ? 2u : 3u;
        }
        p->parts.push_back(kp);
    }
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        int n = 0;
        while (comp_mask[i] >> n & 1u) n++;
        if (comp_mask[i] != (1u << n) - 1u) return "a plane's components must be 0 .. n-1, each fed by one channel";
        p->channels[i] = n;
        p->type[i] = any_float[i] ? RFX_PLANE_F32 : RFX_PLANE_F16;
    }
    return rfx_aov_plan_conv_for(g.W, g.H, g.held_row0, g.held_rows, p->type, p->channels, row0, rows, g.depth_kind, g.velocity_kind, &p->aov);
}

// Coverage of the band's scanlines [y_lo, y_hi) by the blocks of ONE mapped part (first .. last: the rows of each clipped to the band, sorted by
// (lo, hi, x)): every texel in exactly one block.  The x-intervals of a row are sorted and must tile [0, W) — per group of blocks on the same rows
// where such groups follow each other (scanline chunks, tiles), else row by row.
struct ExrSpan { int part, lo, hi, x, cols; };
static const char *exr_cover_row(std::vector<std::pair<int, int>> &iv, int W, const char *overlap, const char *hole) {
    std::sort(iv.begin(), iv.end());
    int x = 0;
    for (const std::pair<int, int> &q : iv) {
        if (q.first < x) return overlap;
        if (q.first > x) return hole;
        x = q.first + q.second;
    }
    return x == W ? nullptr : hole;
}
static const char *exr_cover_part(const ExrSpan *first, const ExrSpan *last, int W, int y_lo, int y_hi, const char *overlap, const char *hole) {
    unsigned long long area = 0;
    for (const ExrSpan *q = first; q != last; q++) area += (unsigned long long)(q->hi - q->lo) * (unsigned long long)q->cols;
    const unsigned long long want = (unsigned long long)(y_hi - y_lo) * (unsigned long long)W;
    if (area != want) return area > want ? overlap : hole;  // (so whatever follows handles at most W x rows texel rows)
    std::vector<std::pair<int, int>> iv;
    bool grouped = true;
    int at = y_lo;
    for (const ExrSpan *g = first; g != last && grouped;) {
        const ExrSpan *e = g;
        while (e != last && e->lo == g->lo && e->hi == g->hi) e++;
        if (g->lo > at) return hole;  // (sorted by lo: nothing later holds scanline `at`)
        grouped = g->lo == at;
        at = g->hi;
        g = e;
    }
    if (grouped) {
        for (const ExrSpan *g = first; g != last;) {
            iv.clear();
            const ExrSpan *e = g;
            for (; e != last && e->lo == g->lo && e->hi == g->hi; e++) iv.push_back({e->x, e->cols});
            if (const char *bad = exr_cover_row(iv, W, overlap, hole)) return bad;
            g = e;
        }
        return nullptr;  // (the groups' rows follow each other from y_lo and the areas add up: they end at y_hi)
    }
    for (int y = y_lo; y < y_hi; y++) {  // blocks of different row ranges side by side
        iv.clear();
        for (const ExrSpan *q = first; q != last && q->lo <= y; q++)
            if (q->hi > y) iv.push_back({q->x, q->cols});
        if (const char *bad = exr_cover_row(iv, W, overlap, hole)) return bad;
    }
    return nullptr;
}

// The blocks: geometry, sizes, the band's blocks and their coverage.  A pure function of the descriptor and the frame's size, after
// exr_parts_plan.  0, or the RFX_EINVAL case in words.
// accept_piz: a PIZ part's blocks are taken (its geometry rules: include/rfx.h "EXR blocks with PIZ"); the parts' plan has refused one otherwise.
static const char *exr_blocks_plan(const ExrGeom &g, unsigned long long file_bytes, const rfx_exr_block *block, int nblocks, int row0, int rows, const char *overlap,
                                   const char *hole, ExrPlan *p, bool accept_piz = false) {
    const int W = g.W, H = g.H, nparts = (int)p->parts.size();
    const int y_lo = H - row0 - rows, y_hi = H - row0;  // the band's scanlines, top first
    std::vector<ExrSpan> spans;
    for (int k = 0; k < nblocks; k++) {
        const rfx_exr_block &q = block[k];
        if (q.part < 0 || q.part >= nparts) return "a block's part";
        const K9Part &part = p->parts[q.part];
        if (q.x < 0 || q.y < 0 || q.cols < 1 || q.rows < 1 || q.x >= W || q.y >= H || q.cols > W - q.x || q.rows > H - q.y) return "a block does not lie inside the frame";
        const unsigned long long texels = (unsigned long long)q.rows * (unsigned long long)q.cols, raw = texels * part.texel_bytes;
        if (raw >= (1ull << 30)) return "a block of 2^30 raw bytes or more";
        if (q.packed_bytes == 0 || q.packed_bytes >= (1ull << 30) || (part.compression == RFX_EXR_NONE && q.packed_bytes != raw)) return "a block's packed size does not fit its texels";
        if (q.offset > file_bytes || q.packed_bytes > file_bytes - q.offset) return "a block lies outside the file bytes";
        int piz = 0;
        if (part.compression == RFX_EXR_PIZ) {
            if (!accept_piz) return "a PIZ part";
            if (q.cols >= 2 * RFX_EXR_PIZ_CELL && q.rows >= 2 * RFX_EXR_PIZ_CELL) return "a PIZ block of 128 x 128 texels or more";
            piz = q.packed_bytes != raw;
        }
        if (!p->mapped[q.part] || q.y >= y_hi || q.y + q.rows <= y_lo) continue;
        const unsigned long long expect = part.compression == RFX_EXR_PXR24 && q.packed_bytes != raw ? texels * part.pxr_bytes : raw;
        if (part.compression == RFX_EXR_RLE && q.packed_bytes != raw) p->rle_chunks++;
        p->chunks.push_back({p->packed_bytes, p->scratch_bytes, (unsigned int)q.packed_bytes, (unsigned int)raw, (unsigned int)expect, q.part, q.x, q.y, q.cols, q.rows, k, piz ? p->piz_chunks : 0});
        p->piz_chunks += piz;
        p->file_offset.push_back(q.offset);
        p->copy_bytes += q.packed_bytes;
        p->packed_bytes += align256(q.packed_bytes);
        p->scratch_bytes += align256(raw);
        spans.push_back({q.part, q.y > y_lo ? q.y : y_lo, q.y + q.rows < y_hi ? q.y + q.rows : y_hi, q.x, q.cols});
    }
    std::sort(spans.begin(), spans.end(), [](const ExrSpan &a, const ExrSpan &b) {
        return a.part != b.part ? a.part < b.part : a.lo != b.lo ? a.lo < b.lo : a.hi != b.hi ? a.hi < b.hi : a.x < b.x;
    });
    size_t at = 0;
    for (int k = 0; k < nparts; k++) {
        if (!p->mapped[k]) continue;
        size_t end = at;
        while (end < spans.size() && spans[end].part == k) end++;
        if (const char *bad = exr_cover_part(spans.data() + at, spans.data() + end, W, y_lo, y_hi, overlap, hole)) return bad;
        at = end;
    }
    return nullptr;
}

// rfx_stage_exr_aov's checks and layout: its own rules for a scanline chunk, then the blocks' plan
static const char *exr_plan(const ExrGeom &g, const rfx_exr_frame *f, int row0, int rows, ExrPlan *p) {
    if (!f->data || !f->bytes || f->parts <= 0 || f->chunks <= 0 || !f->part || !f->chunk) return "an empty descriptor";
    if (f->chunks >= (1 << 23) || f->parts > 4096) return "more than 2^23 chunks or 4096 parts";
    const int W = g.W, H = g.H;
    if (const char *bad = exr_parts_plan(g, f->part, f->parts, 1u << RFX_EXR_NONE | 1u << RFX_EXR_ZIPS | 1u << RFX_EXR_ZIP, "a part's compression is none of NONE, ZIPS, ZIP",
                                         row0, rows, p))
        return bad;
    std::vector<rfx_exr_block> blocks((size_t)f->chunks);
    for (int k = 0; k < f->chunks; k++) {
        const rfx_exr_chunk &q = f->chunk[k];
        if (q.part < 0 || q.part >= f->parts) return "a chunk's part";
        const int per = f->part[q.part].compression == RFX_EXR_ZIP ? 16 : 1;
        if (q.y < 0 || q.y >= H || q.y % per || q.rows != (H - q.y < per ? H - q.y : per)) return "a chunk's scanline or row count does not fit its part's header";
        const unsigned long long raw = (unsigned long long)q.rows * W * p->parts[q.part].texel_bytes;
        if (raw >= (1ull << 30)) return "a chunk of 2^30 raw bytes or more";
        if (q.packed_bytes == 0 || q.packed_bytes >= (1ull << 30) || (f->part[q.part].compression == RFX_EXR_NONE && q.packed_bytes != raw)) return "a chunk's packed size does not fit its rows";
        if (q.offset > f->bytes || q.packed_bytes > f->bytes - q.offset) return "a chunk lies outside the file bytes";
        blocks[(size_t)k] = {q.part, 0, q.y, W, q.rows, 0, q.offset, q.packed_bytes};
    }
    return exr_blocks_plan(g, f->bytes, blocks.data(), f->chunks, row0, rows, "two chunks of a part hold one scanline",
                           "a scanline of the band has no chunk in a part that feeds a plane", p);
}

static const char *exr_block_frame_plan(const ExrGeom &g, const rfx_exr_block_frame *f, int row0, int rows, ExrPlan *p, bool accept_piz = false) {
    if (!f->data || !f->bytes || f->parts <= 0 || f->blocks <= 0 || !f->part || !f->block) return "an empty descriptor";
    if (f->blocks >= (1 << 23) || f->parts > 4096) return "more than 2^23 blocks or 4096 parts";
    const unsigned int five = 1u << RFX_EXR_NONE | 1u << RFX_EXR_RLE | 1u << RFX_EXR_ZIPS | 1u << RFX_EXR_ZIP | 1u << RFX_EXR_PXR24;
    if (const char *bad = exr_parts_plan(g, f->part, f->parts, accept_piz ? five | 1u << RFX_EXR_PIZ : five,
                                         accept_piz ? "a part's compression is none of NONE, RLE, ZIPS, ZIP, PIZ, PXR24" : "a part's compression is none of NONE, RLE, ZIPS, ZIP, PXR24",
                                         row0, rows, p))
        return bad;
    return exr_blocks_plan(g, f->bytes, f->block, f->blocks, row0, rows, "two blocks of a part hold one texel of the band",
                           "a texel of the band has no block in a part that feeds a plane", p, accept_piz);
}

// what every entry point does with a plan: the copies, K9's launches, the status read-back and the pack launches, on the upload stream
static int stage_exr_plan(rfx_ctx *c, const ExrPlan &p, const void *data, const char *fn) {
    const rfx_aov_plan &t = p.aov;
    int rc = stage_plan_begin(c, t, fn);
    if (rc) return rc;
    // the device area: parts | channels | chunks | error words | status | packed bytes | inflate scratch | PIZ tables, every piece 256-byte aligned
    rfx_exr_piz_tables piz;
    if (!rfx_exr_piz_tables_for(p.piz_chunks, &piz)) return fail_in(c, RFX_EINVAL, fn, "too many PIZ blocks");
    const size_t n = p.chunks.size();
    const size_t parts_b = align256(p.parts.size() * sizeof(K9Part)), chans_b = align256(p.chans.size() * sizeof(K9Chan)), chunks_b = align256(n * sizeof(K9Chunk));
    const size_t tables_b = parts_b + chans_b + chunks_b, err_b = align256(n * sizeof(int)), status_b = 256;
    const size_t need = tables_b + err_b + status_b + (size_t)p.packed_bytes + (size_t)p.scratch_bytes + (size_t)piz.bytes;
    if ((rc = grow_stage_area(c, &c->aov_stage, &c->aov_stage_cap, (size_t)t.stage_bytes, (std::string(fn) + ": hipMalloc(staging area)").c_str()))) return rc;
    if ((rc = grow_stage_area(c, &c->exr_stage, &c->exr_stage_cap, need, (std::string(fn) + ": hipMalloc(chunk area)").c_str()))) return rc;
    if (!c->ev_exr_status) {
        hipError_t e = hipEventCreateWithFlags(&c->ev_exr_status, hipEventDisableTiming);
        if (e != hipSuccess) return fail(c, RFX_EDEVICE, (std::string(fn) + ": the status event").c_str(), e);
    }
    if (!c->exr_status_host) {
        hipError_t e = hipHostMalloc((void **)&c->exr_status_host, 2 * sizeof(int), hipHostMallocDefault);
        if (e != hipSuccess) { c->exr_status_host = nullptr; return fail(c, RFX_ENOMEM, (std::string(fn) + ": the status block").c_str(), e); }
    }
    // the tables, written into this batch's pinned block behind what an earlier call of the batch put there
    const int hb = (int)(c->flips & 1u);
    if (c->exr_tables_batch[hb] != c->flips) { c->exr_tables_batch[hb] = c->flips; c->exr_tables_used[hb] = 0; }
    if (c->exr_tables_used[hb] + tables_b > c->exr_tables_cap[hb]) {
        if (c->exr_tables_host[hb]) { HIPCHK(c, hipStreamSynchronize(c->upload_stream)); hipHostFree(c->exr_tables_host[hb]); }  // (grown: as the device areas)
        c->exr_tables_host[hb] = nullptr;
        c->exr_tables_cap[hb] = c->exr_tables_used[hb] = 0;
        hipError_t e = hipHostMalloc(&c->exr_tables_host[hb], 2 * tables_b, hipHostMallocDefault);
        if (e != hipSuccess) return fail(c, RFX_ENOMEM, (std::string(fn) + ": hipHostMalloc(tables)").c_str(), e);
        c->exr_tables_cap[hb] = 2 * tables_b;
    }
    char *tables = (char *)c->exr_tables_host[hb] + c->exr_tables_used[hb];
    c->exr_tables_used[hb] += tables_b;
    memset(tables, 0, tables_b);
    memcpy(tables, p.parts.data(), p.parts.size() * sizeof(K9Part));
    memcpy(tables + parts_b, p.chans.data(), p.chans.size() * sizeof(K9Chan));
    memcpy(tables + parts_b + chans_b, p.chunks.data(), n * sizeof(K9Chunk));
    char *dev = (char *)c->exr_stage;
    // rfx_stage_upload's order: the back buffers were the front buffers until the last flip
    HIPCHK(c, hipStreamWaitEvent(c->upload_stream, c->ev_frame_done, 0));
    HIPCHK(c, hipMemcpyAsync(dev, tables, tables_b, hipMemcpyHostToDevice, c->upload_stream));
    HIPCHK(c, hipMemsetAsync(dev + tables_b + err_b, 0, status_b, c->upload_stream));
    char *packed = dev + tables_b + err_b + status_b;
    for (size_t k = 0; k < n; k++)  // exactly the packed bytes of every chunk the band needs
        HIPCHK(c, hipMemcpyAsync(packed + p.chunks[k].src, (const char *)data + p.file_offset[k], p.chunks[k].packed, hipMemcpyHostToDevice, c->upload_stream));
    K9Args A = {};
    A.parts = (const K9Part *)dev; A.chans = (const K9Chan *)(dev + parts_b); A.chunks = (const K9Chunk *)(dev + parts_b + chans_b);
    A.nchunks = (int)n; A.rle_chunks = p.rle_chunks;
    A.err = (int *)(dev + tables_b); A.status = (int *)(dev + tables_b + err_b);
    A.packed = (const unsigned char *)packed; A.scratch = (unsigned char *)packed + p.packed_bytes;
    A.piz_chunks = p.piz_chunks; A.piz_tables = p.piz_chunks ? A.scratch + p.scratch_bytes : nullptr;
    A.W = c->W; A.H = c->H;
    A.depth_bad_nan = aov_depth_kind(c) != RFX_AOV_DEPTH_FRAGCOORD;  // a bad block reads as not covered: a non-finite view z or position, not depth 1
    A.nseg = t.nseg;
    unsigned int half_mask = 0;
    for (int i = 0; i < RFX_AOV_PLANES; i++) {
        A.plane_ch[i] = p.channels[i];
        A.plane_half[i] = p.channels[i] && p.type[i] == RFX_PLANE_F16;
        if (A.plane_half[i]) half_mask |= 1u << i;
    }
    for (int k = 0; k < t.nseg; k++) {
        A.seg_row0[k] = t.seg[k].row0; A.seg_rows[k] = t.seg[k].rows;
        for (int i = 0; i < RFX_AOV_PLANES; i++) A.seg_plane[k][i] = t.seg[k].offset[i] == ~0ull ? nullptr : (char *)c->aov_stage + t.seg[k].offset[i];
    }
    HIPCHK(c, rfx_launch_k9(A, c->upload_stream));
    HIPCHK(c, hipMemcpyAsync(c->exr_status_host, A.status, 2 * sizeof(int), hipMemcpyDeviceToHost, c->upload_stream));
    HIPCHK(c, hipEventRecord(c->ev_exr_status, c->upload_stream));
    c->exr_staged = true;
    for (int k = 0; k < t.nseg; k++) {
        K0AovArgs P = {};
        for (int i = 0; i < RFX_AOV_PLANES; i++) P.plane[i] = A.seg_plane[k][i];
        P.half_mask = half_mask;
        P.diffuse_ch = p.channels[RFX_AOV_DIFFUSE]; P.direct_ch = p.channels[RFX_AOV_DIRECT];
        HIPCHK(c, aov_pack_segment(c, t, t.seg[k], P));
    }
    stage_plan_end(c, t);
    return RFX_OK;
}

extern "C" {

size_t rfx_exr_aov_stage_bytes(const rfx_ctx *c, const rfx_exr_frame *f, int row0, int rows) {
    ExrPlan p;
    if (!c || !f || exr_plan(exr_geom(c), f, row0, rows, &p)) return 0;
    return (size_t)p.copy_bytes;
}

size_t rfx_exr_blocks_stage_bytes(const rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    ExrPlan p;
    if (!c || !f || exr_block_frame_plan(exr_geom(c), f, row0, rows, &p)) return 0;
    return (size_t)p.copy_bytes;
}

size_t rfx_exr_blocks_piz_stage_bytes(const rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    ExrPlan p;
    if (!c || !f || exr_block_frame_plan(exr_geom(c), f, row0, rows, &p, true)) return 0;
    return (size_t)p.copy_bytes;
}

int rfx_stage_exr_aov(rfx_ctx *c, const rfx_exr_frame *f, int row0, int rows) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    ExrPlan p;
    if (const char *bad = exr_plan(exr_geom(c), f, row0, rows, &p)) return fail_in(c, RFX_EINVAL, "rfx_stage_exr_aov", bad);
    return stage_exr_plan(c, p, f->data, "rfx_stage_exr_aov");
}

int rfx_stage_exr_blocks(rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    ExrPlan p;
    if (const char *bad = exr_block_frame_plan(exr_geom(c), f, row0, rows, &p)) return fail_in(c, RFX_EINVAL, "rfx_stage_exr_blocks", bad);
    return stage_exr_plan(c, p, f->data, "rfx_stage_exr_blocks");
}

int rfx_stage_exr_blocks_piz(rfx_ctx *c, const rfx_exr_block_frame *f, int row0, int rows) {
    if (!c || !f) return RFX_EINVAL;
    RFX_ENTER(c);
    ExrPlan p;
    if (const char *bad = exr_block_frame_plan(exr_geom(c), f, row0, rows, &p, true)) return fail_in(c, RFX_EINVAL, "rfx_stage_exr_blocks_piz", bad);
    return stage_exr_plan(c, p, f->data, "rfx_stage_exr_blocks_piz");
}

int rfx_exr_aov_status(rfx_ctx *c, int *bad_chunks, int *first_bad, int *code) {
    if (!c) return RFX_EINVAL;
    RFX_ENTER(c);
    if (!c->exr_staged) return fail(c, RFX_ESTATE, "rfx_exr_aov_status: no EXR frame has been staged");
    HIPCHK(c, hipEventSynchronize(c->ev_exr_status));
    const int bad = c->exr_status_host[0], key = c->exr_status_host[1] ? 0x7fffffff - c->exr_status_host[1] : -1;
    if (bad_chunks) *bad_chunks = bad;
    if (first_bad) *first_bad = key < 0 ? -1 : key >> 8;
    if (code) *code = key < 0 ? 0 : key & 255;
    return RFX_OK;
}

}  // extern "C"
