// Huffman decode of baseline JPEG scans on the device (include/mpn.h, "JPEG entropy decode on the device"): the file's own
// bytes go over the link, the host only parses headers (mpn_jpeg_scan_prepare in jpeg.hip).
//
// An image's bytes are cut into subsequences of kSub bits, anchored at the image's first byte. A decoder state is (bit
// position over the raw bytes, block index within the MCU, zigzag index); run<>() is f_i: it decodes whole symbols from an
// entry state until the position leaves its subsequence. Huffman streams self-synchronise, so the true entries - the fixed
// point of entry[i + 1] = f_i(entry[i]) from the one known entry at the scan's start - are reached after a few sweeps:
//
//   jpeg_ent_layout_kernel  gives every image its own slots of the workspace (a prefix sum over the descriptors)
//   jpeg_ent_init_kernel    validates the descriptor, zeroes the coefficients, writes the mpn_jpeg_desc, clears the control words
//   jpeg_ent_sync_kernel    x max_passes. A workgroup owns kG subsequences and sweeps them in LDS until no entry changes (at
//                           most kG + 1 sweeps); its exit state is the next group's entry in the NEXT launch, which re-solves
//                           only the subsequences whose entry changed. Entries, exits and counts persist in `work`.
//   jpeg_ent_prefix_kernel  checks the fixed point across groups, exclusive prefix sums of blocks and restart markers
//   jpeg_ent_write_kernel   decodes once more from the true entries and stores coefficients (DC as the difference); every
//                           error condition is judged here
//   jpeg_ent_dc_kernel      per-component running sum of the DC differences in decode order (segmented at restarts); record
//
// No workgroup waits on another; every loop is bounded by nbytes or kG; grids depend on B alone. Decoder state lives in
// registers, the lookahead tables in LDS. The decode core (Reader, run<>, the table steps) is __host__ __device__ so that a
// stand-alone host program can drive it under a sanitizer.
#include "common.h"

namespace {

typedef mpn_jpeg_scan_desc SDesc;
typedef unsigned long long u64;

constexpr int kSub = MPN_JPEG_SUBSEQ_BITS;          // bits per subsequence
constexpr int kSubBytes = kSub / 8;
constexpr int kG = MPN_JPEG_GROUP_SUBSEQ;           // subsequences per group = threads per workgroup
constexpr int kGroupBytes = kG * kSubBytes;
constexpr unsigned kTerminal = 0xFFFFFFFFu;         // the position of a decoder that has seen the end of the scan
constexpr int kLook = 9;
constexpr long long kMaxPixels = 1ll << 28;
constexpr int kInitGroups = 32, kSyncGroups = 32, kWriteGroups = 32;

enum { F_CODE = 1, F_RUN = 2, F_DCCAT = 4, F_TRUNC = 8, F_RESTART = 16, F_COUNT = 32, F_TABLE = 64 };
// control words of an image; C_STATE: -1 skipped, 1 converged; C_SLOT / C_GSLOT: its first subsequence / group slot
enum { C_PASSES = 0, C_FLAGS = 1, C_STATE = 2, C_BLOCKS = 3, C_SLOT = 4, C_GSLOT = 5 };
constexpr int kCtl = 8;

__device__ const uint8_t kNaturalDev[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                            41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                            30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ------------------------------------------------------------------------------------------------ workspace
// control words [B][kCtl] int | carry [2][gslots] u64 | entry, exit, count, first [slots] u64 each. Image b's subsequences
// take the slots behind those of the images before it IN DESCRIPTOR ORDER (jpeg_ent_layout_kernel: an exclusive prefix sum of
// ceil(nbytes / kSubBytes) over the descriptors), its groups likewise: no two images share a slot, wherever their files lie
// and in whatever order. Files that do not overlap need at most files_bytes / kSubBytes + B slots; an image whose slots would
// reach past the workspace (descriptors that name the same bytes more than once can do that) is skipped.
struct Layout {
    long long slots, gslots;
    size_t carry, entry, exit, count, first, bytes;
};

__host__ __device__ inline Layout layout_of(int B, unsigned long long files_bytes) {
    Layout l;
    l.slots = (long long)(files_bytes / kSubBytes) + B + 1;
    l.gslots = (long long)(files_bytes / kGroupBytes) + B + 1;
    l.carry = (size_t)B * kCtl * 4;
    l.entry = l.carry + (size_t)l.gslots * 16;
    l.exit = l.entry + (size_t)l.slots * 8;
    l.count = l.exit + (size_t)l.slots * 8;
    l.first = l.count + (size_t)l.slots * 8;
    l.bytes = l.first + (size_t)l.slots * 8;
    return l;
}

struct Work {
    int* ctl;
    u64* carry0;
    long long gslots;
    __device__ __forceinline__ u64* carry(int pass) const { return carry0 + (pass & 1) * gslots; }      // the buffer pass `pass` writes
    u64 *entry, *exit, *count, *first;
};

__device__ __forceinline__ Work work_of(uint8_t* work, const Layout& l) {
    Work w;
    w.ctl = reinterpret_cast<int*>(work);
    w.carry0 = reinterpret_cast<u64*>(work + l.carry);
    w.gslots = l.gslots;
    w.entry = reinterpret_cast<u64*>(work + l.entry);
    w.exit = reinterpret_cast<u64*>(work + l.exit);
    w.count = reinterpret_cast<u64*>(work + l.count);
    w.first = reinterpret_cast<u64*>(work + l.first);
    return w;
}

// ------------------------------------------------------------------------------------------------ descriptor
struct Img {
    const uint8_t* data;
    unsigned nbytes, scan_bit;
    int nsub, first, ngroups, gfirst;       // subsequences of the file; the one that holds the scan's first bit; groups
    long long slot0, gslot0;
    int ncomp, hv, bpm, hs, vs, total, mcus_x, restart;
    int bw0, bwc, base1, base2;             // blocks per row of the luma / a chroma plane; first block of the chroma planes
};

// Everything the kernels touch for an image, from its descriptor alone: false = the image is skipped.
__host__ __device__ __forceinline__ bool image_of(const SDesc& d, int b, const uint8_t* files, size_t files_bytes, size_t coef_bytes,
                                                  const Layout& l, const int* ctl, Img& im) {
    if (d.width < 1 || d.height < 1 || d.width > 65535 || d.height > 65535 || (long long)d.width * d.height > kMaxPixels) return false;
    if (d.components != 1 && d.components != 3) return false;
    const bool samp_ok = (d.h_samp == 1 && d.v_samp == 1) || (d.components == 3 && d.h_samp == 2 && (d.v_samp == 1 || d.v_samp == 2));
    if (!samp_ok) return false;
    im.ncomp = d.components;
    im.hs = d.h_samp;
    im.vs = d.v_samp;
    im.hv = im.hs * im.vs;
    im.bpm = im.ncomp == 3 ? im.hv + 2 : 1;
    const int mx = (d.width + 8 * im.hs - 1) / (8 * im.hs), my = (d.height + 8 * im.vs - 1) / (8 * im.vs);
    im.mcus_x = mx;
    im.bw0 = mx * im.hs;
    im.bwc = im.ncomp == 3 ? mx : 0;
    im.base1 = im.bw0 * my * im.vs;
    im.base2 = im.base1 + im.bwc * my;
    im.total = im.base2 + im.bwc * my;
    if (d.restart_interval < 0 || d.restart_interval > 65535) return false;
    im.restart = d.restart_interval;
    for (int c = 0; c < 3; ++c) {
        if (d.dc_table[c] < 0 || d.dc_table[c] > 3 || d.ac_table[c] < 0 || d.ac_table[c] > 3) return false;
    }
    if (d.file_offset < 0 || d.coef_offset < 0 || ((d.file_offset | d.coef_offset) & 15)) return false;
    if (d.nbytes < 1 || d.nbytes > MPN_JPEG_MAX_FILE_BYTES || d.scan_offset < 0 || d.scan_offset > d.nbytes) return false;
    if ((unsigned long long)d.file_offset + (unsigned long long)d.nbytes > files_bytes) return false;
    if ((unsigned long long)d.coef_offset + (unsigned long long)im.total * 128ull > coef_bytes) return false;
    im.data = files + d.file_offset;
    im.nbytes = (unsigned)d.nbytes;
    im.scan_bit = (unsigned)d.scan_offset * 8u;
    im.nsub = (int)((im.nbytes + kSubBytes - 1) / kSubBytes);
    im.first = (int)(im.scan_bit / kSub);
    if (im.first >= im.nsub) im.first = im.nsub - 1;           // (scan_offset == nbytes on a multiple of kSubBytes: an empty scan)
    im.ngroups = (im.nsub + kG - 1) / kG;
    im.gfirst = im.first / kG;
    im.slot0 = ctl[b * kCtl + C_SLOT];
    im.gslot0 = ctl[b * kCtl + C_GSLOT];
    return im.slot0 >= 0 && im.gslot0 >= 0 && im.slot0 + im.nsub <= l.slots && im.gslot0 + im.ngroups <= l.gslots;
}

// Plane position (in blocks) of block `blk` of the decode order.
__host__ __device__ __forceinline__ int block_index(const Img& im, unsigned blk) {
    const unsigned mcu = blk / (unsigned)im.bpm, bi = blk - mcu * (unsigned)im.bpm;
    const unsigned my = mcu / (unsigned)im.mcus_x, mx = mcu - my * (unsigned)im.mcus_x;
    if (bi < (unsigned)im.hv) {
        const unsigned v = bi / (unsigned)im.hs, h = bi - v * (unsigned)im.hs;
        return (int)((my * im.vs + v) * im.bw0 + mx * im.hs + h);
    }
    return (bi == (unsigned)im.hv ? im.base1 : im.base2) + (int)(my * im.bwc + mx);
}

// ------------------------------------------------------------------------------------------------ tables (LDS)
struct Tab {
    uint16_t look[1 << kLook];      // (code length << 8) | symbol of the code that starts these 9 bits; 0 = longer than 9
    int maxcode[17];                // largest code of each length (-1: none)
    int valoff[17];                 // index of a length's first symbol minus its first code
    uint8_t vals[256];
};

struct Shared {
    Tab tabs[6];                    // [component][DC, AC]
    uint8_t natural[64];
};

// Do the counts of a table (codes of length 1..16) form a prefix code of at most 256 symbols?
__host__ __device__ __forceinline__ bool counts_are_prefix_code(const uint8_t* bits) {
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        code += bits[l - 1];
        k += bits[l - 1];
        if (code > (1 << l) || k > 256) return false;
        code <<= 1;
    }
    return true;
}

// The two steps of a table, one call per table / per lookahead entry. table_lengths: false when the counts are no prefix code.
__host__ __device__ __forceinline__ bool table_lengths(const uint8_t* bits, Tab& t) {
    bool ok = true;
    int code = 0, k = 0;
    t.maxcode[0] = -1;
    t.valoff[0] = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valoff[l] = k - code;
        code += bits[l - 1];
        k += bits[l - 1];
        if (code > (1 << l) || k > 256) ok = false;
        t.maxcode[l] = bits[l - 1] ? code - 1 : -1;
        code <<= 1;
    }
    return ok;
}

__host__ __device__ __forceinline__ uint16_t look_entry(const Tab& t, int v) {
    for (int l = 1; l <= kLook; ++l) {
        const int code = v >> (kLook - l);
        if (code <= t.maxcode[l]) return (uint16_t)(((unsigned)l << 8) | t.vals[(code + t.valoff[l]) & 255]);
    }
    return 0;
}

// All threads of the workgroup. Returns false (to every thread) when a table is not a prefix code: the init kernel has
// reported that already (F_TABLE), and the sync and write kernels go on with the table as built - every index into it is
// masked and every loop bounded, so such a table costs time, not safety.
__device__ bool build_tables(const SDesc& d, int ncomp, Shared& sh) {
    __shared__ int bad;
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) bad = 0;
    __syncthreads();
    if (tid < 2 * ncomp) {
        const int c = tid >> 1, cls = tid & 1;
        if (!table_lengths(d.huff_bits[cls][(cls ? d.ac_table[c] : d.dc_table[c]) & 3], sh.tabs[tid])) bad = 1;
    }
    for (int i = tid; i < 2 * ncomp * 256; i += nt) {
        const int t = i >> 8, c = t >> 1, cls = t & 1;
        sh.tabs[t].vals[i & 255] = d.huff_vals[cls][(cls ? d.ac_table[c] : d.dc_table[c]) & 3][i & 255];
    }
    if (tid < 64) sh.natural[tid] = kNaturalDev[tid];
    __syncthreads();
    for (int i = tid; i < 2 * ncomp * (1 << kLook); i += nt) {
        Tab& t = sh.tabs[i >> kLook];
        t.look[i & ((1 << kLook) - 1)] = look_entry(t, i & ((1 << kLook) - 1));
    }
    __syncthreads();
    return bad == 0;
}

// ------------------------------------------------------------------------------------------------ bit reader
// The entropy-coded bytes as a bit stream: `n` unread bits in the low end of `buf`. A stuffed 00 is dropped on the way in and
// remembered in `sm` (a bit beside the last bit of its FF), so that the RAW bit position of the next unread bit is known at
// any time; a marker or the end of the data stops the input and zero bits follow, counted in `fake`.
struct Reader {
    const uint8_t* data;
    unsigned nbytes, bp, after;     // bp: next byte to fetch (the marker's FF once stopped); after: first byte behind an RSTn
    u64 buf, sm;
    int n, fake, stop;              // stop: 0 reading, 1 at an RSTn marker, 2 at another marker, 3 at the end of the data

    __host__ __device__ __forceinline__ void refill() {
        while (n <= 56) {
            if (stop) {
                buf <<= 8;
                sm <<= 8;
                n += 8;
                fake += 8;
                continue;
            }
            if (bp >= nbytes) {
                stop = 3;
                continue;
            }
            const unsigned c = data[bp];
            if (c != 0xFFu) {
                buf = (buf << 8) | c;
                sm <<= 8;
                n += 8;
                ++bp;
                continue;
            }
            unsigned j = bp + 1;
            if (j < nbytes && data[j] == 0) {
                buf = (buf << 8) | 0xFFu;
                sm = (sm << 8) | 1u;
                n += 8;
                bp += 2;
                continue;
            }
            while (j < nbytes && data[j] == 0xFFu) ++j;         // fill bytes in front of a marker
            if (j >= nbytes) {
                stop = 3;
            } else if (data[j] >= 0xD0u && data[j] <= 0xD7u) {
                stop = 1;
                after = j + 1;
            } else {
                stop = 2;
            }
        }
    }
    __host__ __device__ __forceinline__ void start(unsigned pos) {
        bp = pos >> 3;
        after = 0;
        buf = sm = 0;
        n = fake = stop = 0;
        refill();
        n -= (int)(pos & 7u);
    }
    __host__ __device__ __forceinline__ unsigned pos() const {            // n >= fake
        const u64 mask = n >= 64 ? ~0ull : ((1ull << n) - 1ull);
        return bp * 8u - (unsigned)(n - fake) - 8u * (unsigned)__builtin_popcountll(sm & mask);
    }
    // Stopped, and what is left of the last byte is its padding: fewer than 8 bits, all of them 1 (no Huffman code is all ones).
    __host__ __device__ __forceinline__ bool padding() const {
        const int real = n - fake;
        if (real <= 0) return true;
        if (real >= 8) return false;
        const unsigned ones = (1u << real) - 1u;
        return ((unsigned)(buf >> fake) & ones) == ones;
    }
    __host__ __device__ __forceinline__ unsigned get(int s) {            // 1 <= s <= 16 <= n
        n -= s;
        return (unsigned)(buf >> n) & ((1u << s) - 1u);
    }
    __host__ __device__ __forceinline__ int decode(const Tab& t) {       // n >= 32
        const unsigned e = t.look[(unsigned)(buf >> (n - kLook)) & ((1u << kLook) - 1u)];
        if (e) {
            n -= (int)(e >> 8);
            return (int)(e & 255u);
        }
        int l = kLook + 1;
        int code = (int)((buf >> (n - l)) & ((1u << l) - 1u));
        while (l <= 16 && code > t.maxcode[l]) {
            ++l;
            code = (int)((buf >> (n - l)) & ((1u << l) - 1u));
        }
        if (l > 16) return -1;
        n -= l;
        return t.vals[(code + t.valoff[l]) & 255];
    }
};

__host__ __device__ __forceinline__ int extend(unsigned v, int s) { return v < (1u << (s - 1)) ? (int)v - (1 << s) + 1 : (int)v; }

struct Exit {
    unsigned pos, bz, blocks, restarts;
};

// f_i: decodes from (pos, bz = block << 6 | zigzag) until the position reaches `end`. kFinal: the entry is a true one; blocks
// are stored from block blk0 of the decode order on (rst0 markers were passed before), and errors are collected in `flags`.
// Every iteration consumes at least one bit, so kSub + 8 iterations bound the loop.
template <bool kFinal>
__host__ __device__ __forceinline__ Exit run(const Img& im, const Shared& sh, unsigned pos, unsigned bz, unsigned end, int16_t* coefs,
                                    unsigned blk0, unsigned rst0, int& flags) {
    Exit x = {pos, bz, 0u, 0u};
    if (pos >= end) return x;
    Reader r;
    r.data = im.data;
    r.nbytes = im.nbytes;
    r.start(pos);
    int b = (int)(bz >> 6), z = (int)(bz & 63u);
    if (b >= im.bpm) b = 0;
    int16_t* out = nullptr;
    if (kFinal && blk0 < (unsigned)im.total) out = coefs + (size_t)block_index(im, blk0) * 64;
    for (int it = 0; it < kSub + 8; ++it) {
        if (r.n < 32) r.refill();
        if (r.stop && r.padding()) {                            // only the padding of the last byte is left
            if (r.stop == 1) {                                  // RSTn: align behind it, reset
                if (kFinal) {
                    const u64 want = (u64)(rst0 + x.restarts + 1u) * (u64)im.restart * (u64)im.bpm;
                    if ((b | z) || im.restart == 0 || (u64)(blk0 + x.blocks) != want) flags |= F_RESTART;
                }
                ++x.restarts;
                b = z = 0;
                x.pos = r.after * 8u;
                if (x.pos >= end) {
                    x.bz = 0;
                    return x;
                }
                r.start(x.pos);
                continue;
            }
            if (kFinal) {
                if (r.stop == 3) flags |= F_TRUNC;              // the data ends without a marker
                if (b | z) flags |= F_COUNT;
            }
            x.pos = kTerminal;
            x.bz = 0;
            return x;
        }
        x.pos = r.pos();
        if (x.pos >= end) {
            x.bz = ((unsigned)b << 6) | (unsigned)z;
            return x;
        }
        const int c = b < im.hv ? 0 : 1 + b - im.hv;
        if (z == 0) {
            int s = r.decode(sh.tabs[2 * c]);
            if (s < 0) {                                        // an invalid code consumes one bit
                if (kFinal) flags |= F_CODE;
                r.n -= 1;
                s = 0;
            }
            if (kFinal && s > 11) flags |= F_DCCAT;
            s &= 15;
            int v = 0;
            if (s) v = extend(r.get(s), s);
            if (kFinal) {
                if (out) out[0] = (int16_t)v;
                else flags |= F_COUNT;                          // more blocks than the image has
            }
            z = 1;
        } else {
            const int rs = r.decode(sh.tabs[2 * c + 1]);
            if (rs < 0) {
                if (kFinal) flags |= F_CODE;
                r.n -= 1;
            } else {
                const int run = rs >> 4, s = rs & 15;
                if (s) {
                    z += run;
                    if (z > 63) {
                        if (kFinal) flags |= F_RUN;
                        z = 63;
                    }
                    const int v = extend(r.get(s), s);
                    if (kFinal && out) out[sh.natural[z]] = (int16_t)v;
                    ++z;
                } else {
                    z = run == 15 ? z + 16 : 64;
                }
            }
        }
        if (r.n < r.fake) {                                     // bits that are not in the stream were consumed
            if (kFinal) flags |= F_TRUNC;
            x.pos = kTerminal;
            x.bz = 0;
            return x;
        }
        if (z >= 64) {
            z = 0;
            ++x.blocks;
            if (++b == im.bpm) b = 0;
            if (kFinal) {
                const unsigned blk = blk0 + x.blocks;
                out = blk < (unsigned)im.total ? coefs + (size_t)block_index(im, blk) * 64 : nullptr;
            }
        }
    }
    x.pos = kTerminal;                                          // (not reached from an entry inside the subsequence)
    x.bz = 0;
    return x;
}

__host__ __device__ __forceinline__ u64 pack(unsigned lo, unsigned hi) { return (u64)lo | ((u64)hi << 32); }

// ------------------------------------------------------------------------------------------------ kernels
// One workgroup: every image's first subsequence slot and first group slot, exclusive prefix sums over the descriptors in
// chunks of kG (a descriptor whose nbytes is out of range takes none: its image is skipped anyway).
__global__ void __launch_bounds__(kG) jpeg_ent_layout_kernel(const SDesc* __restrict__ descs, int B, size_t files_bytes,
                                                             uint8_t* __restrict__ work) {
    __shared__ u64 subs[kG], groups[kG];
    const int t = threadIdx.x;
    const Layout l = layout_of(B, files_bytes);
    int* ctl = reinterpret_cast<int*>(work);
    u64 sub_base = 0, group_base = 0;
    for (int base = 0; base < B; base += kG) {                                  // (uniform trip count)
        const int b = base + t;
        u64 nsub = 0, ngroups = 0;
        if (b < B) {
            const long long n = descs[b].nbytes;
            if (n >= 1 && n <= MPN_JPEG_MAX_FILE_BYTES) {
                nsub = (u64)((n + kSubBytes - 1) / kSubBytes);
                ngroups = (nsub + kG - 1) / kG;
            }
        }
        subs[t] = nsub;
        groups[t] = ngroups;
        __syncthreads();
        for (int step = 1; step < kG; step <<= 1) {                            // inclusive scans (65535 files of 2^21: no overflow)
            const u64 s = t >= step ? subs[t - step] : 0ull, g = t >= step ? groups[t - step] : 0ull;
            __syncthreads();
            subs[t] += s;
            groups[t] += g;
            __syncthreads();
        }
        if (b < B) {
            const u64 slot = sub_base + subs[t] - nsub, gslot = group_base + groups[t] - ngroups;
            ctl[b * kCtl + C_SLOT] = slot <= (u64)l.slots ? (int)slot : -1;     // (slots < 2^31: files_bytes < 2^31)
            ctl[b * kCtl + C_GSLOT] = gslot <= (u64)l.gslots ? (int)gslot : -1;
        }
        sub_base += subs[kG - 1];
        group_base += groups[kG - 1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kG) jpeg_ent_init_kernel(const uint8_t* __restrict__ files, size_t files_bytes,
                                                           const SDesc* __restrict__ descs, int B, int16_t* __restrict__ coefs,
                                                           size_t coef_bytes, mpn_jpeg_desc* __restrict__ out, uint8_t* __restrict__ work) {
    __shared__ mpn_jpeg_desc sd;
    const int b = blockIdx.y;
    const SDesc& d = descs[b];
    const Layout l = layout_of(B, files_bytes);
    Work w = work_of(work, l);
    Img im;
    const bool ok = image_of(d, b, files, files_bytes, coef_bytes, l, w.ctl, im);      // (uniform over the workgroup)
    if (blockIdx.x == 0) {
        int* words = reinterpret_cast<int*>(&sd);
        for (int i = threadIdx.x; i < (int)(sizeof(sd) / 4); i += kG) words[i] = 0;
        __syncthreads();
        int bad_table = 0;
        if (ok && threadIdx.x < 2 * im.ncomp) {
            const int c = threadIdx.x >> 1, cls = threadIdx.x & 1;
            bad_table = !counts_are_prefix_code(d.huff_bits[cls][(cls ? d.ac_table[c] : d.dc_table[c]) & 3]);
        }
        const bool tables = !__syncthreads_or(bad_table);
        if (threadIdx.x == 0) {
            if (ok) {
                sd.src_offset = d.src_offset;
                sd.coef_offset = d.coef_offset;
                sd.work_offset = d.work_offset;
                sd.width = d.width;
                sd.height = d.height;
                sd.components = d.components;
                sd.h_samp = d.h_samp;
                sd.v_samp = d.v_samp;
                sd.total_blocks = im.total;
                const int my = (d.height + 8 * im.vs - 1) / (8 * im.vs);
                for (int c = 0; c < im.ncomp; ++c) {
                    sd.blocks_w[c] = c == 0 ? im.bw0 : im.bwc;
                    sd.blocks_h[c] = c == 0 ? my * im.vs : my;
                }
            }
            w.ctl[b * kCtl + C_PASSES] = 0;
            w.ctl[b * kCtl + C_FLAGS] = tables ? 0 : F_TABLE;
            w.ctl[b * kCtl + C_STATE] = ok ? 0 : -1;
            w.ctl[b * kCtl + C_BLOCKS] = 0;
        }
        __syncthreads();
        if (ok) {
            for (int i = threadIdx.x; i < im.ncomp * 64; i += kG) sd.quant[i >> 6][i & 63] = d.quant[i >> 6][i & 63];
        }
        __syncthreads();
        int* dst = reinterpret_cast<int*>(out + b);
        for (int i = threadIdx.x; i < (int)(sizeof(sd) / 4); i += kG) dst[i] = words[i];
    }
    if (!ok) return;
    uint4* z = reinterpret_cast<uint4*>(reinterpret_cast<uint8_t*>(coefs) + d.coef_offset);     // (16-byte aligned, 128 per block)
    const unsigned n16 = (unsigned)im.total * 8u;
    for (unsigned i = blockIdx.x * kG + threadIdx.x; i < n16; i += gridDim.x * kG) z[i] = make_uint4(0u, 0u, 0u, 0u);
}

__global__ void __launch_bounds__(kG) jpeg_ent_sync_kernel(const uint8_t* __restrict__ files, size_t files_bytes,
                                                           const SDesc* __restrict__ descs, int B, size_t coef_bytes,
                                                           uint8_t* __restrict__ work, int pass) {
    __shared__ Shared sh;
    __shared__ unsigned e_pos[kG + 1], e_bz[kG + 1];
    const int b = blockIdx.y, t = threadIdx.x;
    const SDesc& d = descs[b];
    const Layout l = layout_of(B, files_bytes);
    Work w = work_of(work, l);
    Img im;
    if (!image_of(d, b, files, files_bytes, coef_bytes, l, w.ctl, im)) return;
    bool built = false;
    int unused = 0;
    for (int grp = im.gfirst + (int)blockIdx.x; grp < im.ngroups; grp += (int)gridDim.x) {      // (uniform over the workgroup)
        const int i = grp * kG + t;
        const bool active = i >= im.first && i < im.nsub;
        const long long slot = im.slot0 + i;
        const int last = min(im.nsub, (grp + 1) * kG) - 1;                     // the group's last subsequence
        // the group's entry: known for the group that holds the scan's start, else the previous group's exit of the pass before
        u64 carry = 0;
        bool changed = pass == 1;
        if (grp > im.gfirst) {
            carry = pass == 1 ? pack((unsigned)(grp * kG) * (unsigned)kSub, 0u) : w.carry(pass - 1)[im.gslot0 + grp];
            if (pass > 1) changed = carry != w.entry[im.slot0 + grp * kG];
        }
        if (!changed) {                                                         // nothing to re-solve: hand the exit on
            if (t == 0 && grp + 1 < im.ngroups) w.carry(pass)[im.gslot0 + grp + 1] = w.exit[im.slot0 + last];
            continue;
        }
        if (!built) {
            build_tables(d, im.ncomp, sh);
            built = true;
        }
        u64 mine = 0;                                                           // the entry `x` was computed from
        bool have = false;
        Exit x = {0u, 0u, 0u, 0u};
        if (active) {
            u64 e;
            if (i == im.first) {
                e = pack(im.scan_bit, 0u);
            } else if (t == 0) {
                e = carry;
            } else if (pass == 1) {
                e = pack((unsigned)i * (unsigned)kSub, 0u);
            } else {
                e = w.entry[slot];
            }
            if (pass > 1) {
                mine = w.entry[slot];
                have = true;
                const u64 ex = w.exit[slot], cn = w.count[slot];
                x.pos = (unsigned)ex;
                x.bz = (unsigned)(ex >> 32);
                x.blocks = (unsigned)cn;
                x.restarts = (unsigned)(cn >> 32);
            }
            e_pos[t] = (unsigned)e;
            e_bz[t] = (unsigned)(e >> 32);
        }
        __syncthreads();
        for (int sweep = 0; sweep <= kG; ++sweep) {
            bool ch = false;
            if (active) {
                const u64 in = pack(e_pos[t], e_bz[t]);
                ch = !have || in != mine;
                if (ch) {
                    x = run<false>(im, sh, (unsigned)in, (unsigned)(in >> 32), (unsigned)(i + 1) * (unsigned)kSub, nullptr, 0u, 0u, unused);
                    mine = in;
                    have = true;
                }
            }
            __syncthreads();                                                    // every entry has been read
            if (ch) {
                e_pos[t + 1] = x.pos;
                e_bz[t + 1] = x.bz;
            }
            if (!__syncthreads_or(ch)) break;
        }
        if (active) {
            w.entry[slot] = mine;
            w.exit[slot] = pack(x.pos, x.bz);
            w.count[slot] = pack(x.blocks, x.restarts);
            if (i == last && grp + 1 < im.ngroups) w.carry(pass)[im.gslot0 + grp + 1] = pack(x.pos, x.bz);
        }
        if (t == 0) atomicMax(&w.ctl[b * kCtl + C_PASSES], pass);
        __syncthreads();                                                        // the entries in LDS are reused by the next group
    }
}

// One workgroup per image: is the last pass a fixed point across groups; exclusive prefix sums of (blocks, restart markers).
__global__ void __launch_bounds__(kG) jpeg_ent_prefix_kernel(const uint8_t* __restrict__ files, size_t files_bytes,
                                                             const SDesc* __restrict__ descs, int B, size_t coef_bytes,
                                                             uint8_t* __restrict__ work, int passes) {
    __shared__ u64 sums[kG];
    const int b = blockIdx.x, t = threadIdx.x;
    const SDesc& d = descs[b];
    const Layout l = layout_of(B, files_bytes);
    Work w = work_of(work, l);
    Img im;
    if (!image_of(d, b, files, files_bytes, coef_bytes, l, w.ctl, im)) return;
    int differs = 0;
    for (int grp = im.gfirst + 1 + t; grp < im.ngroups; grp += kG) {
        differs |= w.carry(passes)[im.gslot0 + grp] != w.entry[im.slot0 + grp * kG];
    }
    const int open = __syncthreads_or(differs);
    u64 running = 0;
    for (int base = im.first; base < im.nsub; base += kG) {                     // (uniform trip count)
        const int i = base + t;
        const u64 own = i < im.nsub ? w.count[im.slot0 + i] : 0ull;
        sums[t] = own;
        __syncthreads();
        for (int step = 1; step < kG; step <<= 1) {                            // inclusive scan; both halves add without a carry
            const u64 other = t >= step ? sums[t - step] : 0ull;                // between them: blocks stay far below 2^32
            __syncthreads();
            sums[t] += other;
            __syncthreads();
        }
        if (i < im.nsub) w.first[im.slot0 + i] = running + sums[t] - own;
        running += sums[kG - 1];
        __syncthreads();
    }
    if (t == 0) {
        const unsigned blocks = (unsigned)running, restarts = (unsigned)(running >> 32);
        const unsigned mcus = (unsigned)(im.total / im.bpm);
        const unsigned want = im.restart ? (mcus - 1u) / (unsigned)im.restart : 0u;
        w.ctl[b * kCtl + C_BLOCKS] = (int)blocks;
        if (!open) {
            w.ctl[b * kCtl + C_STATE] = 1;
            if (blocks != (unsigned)im.total || restarts != want) atomicOr(&w.ctl[b * kCtl + C_FLAGS], F_COUNT);
        }
    }
}

__global__ void __launch_bounds__(kG) jpeg_ent_write_kernel(const uint8_t* __restrict__ files, size_t files_bytes,
                                                            const SDesc* __restrict__ descs, int B, int16_t* __restrict__ coefs,
                                                            size_t coef_bytes, uint8_t* __restrict__ work) {
    __shared__ Shared sh;
    const int b = blockIdx.y, t = threadIdx.x;
    const SDesc& d = descs[b];
    const Layout l = layout_of(B, files_bytes);
    Work w = work_of(work, l);
    Img im;
    if (!image_of(d, b, files, files_bytes, coef_bytes, l, w.ctl, im)) return;
    if (w.ctl[b * kCtl + C_STATE] != 1) return;                                    // (uniform: written by the launch before)
    build_tables(d, im.ncomp, sh);
    int16_t* mine = coefs + d.coef_offset / 2;
    int flags = 0;
    for (int i = im.first + (int)blockIdx.x * kG + t; i < im.nsub; i += (int)gridDim.x * kG) {
        const long long slot = im.slot0 + i;
        const u64 e = i == im.first ? pack(im.scan_bit, 0u) : w.entry[slot], f = w.first[slot];
        run<true>(im, sh, (unsigned)e, (unsigned)(e >> 32), (unsigned)(i + 1) * (unsigned)kSub, mine, (unsigned)f, (unsigned)(f >> 32), flags);
    }
    if (flags) atomicOr(&w.ctl[b * kCtl + C_FLAGS], flags);
}

// Workgroup (c, b): the running sum of component c's DC differences in decode order, a new segment every restart_interval
// MCUs. A segmented inclusive scan per 256 blocks, the last value carried into the next 256. Workgroup (0, b) writes the record.
__global__ void __launch_bounds__(kG) jpeg_ent_dc_kernel(const uint8_t* __restrict__ files, size_t files_bytes,
                                                         const SDesc* __restrict__ descs, int B, int16_t* __restrict__ coefs,
                                                         size_t coef_bytes, uint8_t* __restrict__ work,
                                                         mpn_jpeg_entropy_record* __restrict__ records) {
    __shared__ unsigned val[kG];
    __shared__ int head[kG];
    const int b = blockIdx.y, c = blockIdx.x, t = threadIdx.x;
    const SDesc& d = descs[b];
    const Layout l = layout_of(B, files_bytes);
    Work w = work_of(work, l);
    const int state = w.ctl[b * kCtl + C_STATE], flags = w.ctl[b * kCtl + C_FLAGS];
    if (c == 0 && t == 0) {
        mpn_jpeg_entropy_record r = {MPN_JPEG_ENT_OK, w.ctl[b * kCtl + C_PASSES], w.ctl[b * kCtl + C_BLOCKS], 0};
        if (state < 0) {
            r.status = MPN_JPEG_ENT_SKIPPED;
            r.passes = r.blocks = 0;
        } else if (flags & F_TABLE) {
            r.status = MPN_JPEG_ENT_BAD_DATA;
        } else if (state != 1) {
            r.status = MPN_JPEG_ENT_NOT_CONVERGED;
        } else if (flags) {
            r.status = MPN_JPEG_ENT_BAD_DATA;
        }
        records[b] = r;
    }
    Img im;
    if (state != 1 || !image_of(d, b, files, files_bytes, coef_bytes, l, w.ctl, im) || c >= im.ncomp) return;
    int16_t* mine = coefs + d.coef_offset / 2;
    const unsigned per = c == 0 ? (unsigned)im.hv : 1u;
    const unsigned count = (unsigned)(im.total / im.bpm) * per;
    unsigned carry = 0;
    for (unsigned base = 0; base < count; base += kG) {                         // (uniform trip count)
        const unsigned j = base + t;
        int16_t* at = nullptr;
        unsigned v = 0;
        int h = 0;
        if (j < count) {
            const unsigned mcu = j / per, bi = j - mcu * per;
            at = mine + (size_t)block_index(im, mcu * (unsigned)im.bpm + (c == 0 ? bi : (unsigned)im.hv + (unsigned)(c - 1))) * 64;
            v = (unsigned)(int)*at;
            h = im.restart && bi == 0 && mcu % (unsigned)im.restart == 0;
        }
        val[t] = v;
        head[t] = h;
        __syncthreads();
        for (int step = 1; step < kG; step <<= 1) {
            unsigned ov = 0;
            int oh = 0;
            if (t >= step) {
                ov = val[t - step];
                oh = head[t - step];
            }
            __syncthreads();
            if (t >= step && !head[t]) {
                val[t] += ov;
                head[t] = oh;
            }
            __syncthreads();
        }
        const unsigned sum = head[t] ? val[t] : val[t] + carry;
        if (at) *at = (int16_t)sum;
        __syncthreads();
        if (t == kG - 1) val[0] = sum;
        __syncthreads();
        carry = val[0];
        __syncthreads();
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------------ entry points
extern "C" size_t mpn_jpeg_entropy_decode_device_workspace_bytes(int B, long long total_file_bytes) {
    if (B < 1 || B > 65535 || total_file_bytes < 16 || total_file_bytes >= (1ll << 31)) return 0;
    return (layout_of(B, (unsigned long long)total_file_bytes).bytes + 15) & ~(size_t)15;
}

extern "C" int mpn_jpeg_entropy_decode_device(const uint8_t* files, size_t files_bytes, const void* scan_descs, int B, int16_t* coefs,
                                              size_t coef_bytes, void* jpeg_descs_out, void* records, void* work, size_t work_bytes,
                                              int max_passes, mpn_stream_t stream) {
    MPN_REQUIRE(files && scan_descs && coefs && jpeg_descs_out && records && work, MPN_ERR_BAD_ARG, "jpeg_entropy_decode_device: null pointer");
    MPN_REQUIRE(B >= 1 && B <= 65535, MPN_ERR_BAD_SHAPE, "jpeg_entropy_decode_device: B must be in [1, 65535] (got %d)", B);
    MPN_REQUIRE(max_passes >= 1 && max_passes <= MPN_JPEG_MAX_PASSES, MPN_ERR_BAD_SHAPE,
                "jpeg_entropy_decode_device: max_passes must be in [1, %d] (got %d)", MPN_JPEG_MAX_PASSES, max_passes);
    MPN_REQUIRE(mpn_aligned16(files) && mpn_aligned16(scan_descs) && mpn_aligned16(coefs) && mpn_aligned16(jpeg_descs_out) &&
                    mpn_aligned16(records) && mpn_aligned16(work),
                MPN_ERR_BAD_ALIGN, "jpeg_entropy_decode_device: files, scan_descs, coefs, jpeg_descs_out, records and work must be 16-byte aligned");
    MPN_REQUIRE(files_bytes >= 16 && files_bytes < ((size_t)1 << 31) && coef_bytes >= 128, MPN_ERR_WORKSPACE,
                "jpeg_entropy_decode_device: files of %zu, coefficients of %zu bytes", files_bytes, coef_bytes);
    const size_t need = mpn_jpeg_entropy_decode_device_workspace_bytes(B, (long long)files_bytes);
    MPN_REQUIRE(work_bytes >= need, MPN_ERR_WORKSPACE, "jpeg_entropy_decode_device: workspace of %zu bytes < %zu", work_bytes, need);
    const SDesc* dd = reinterpret_cast<const SDesc*>(scan_descs);
    uint8_t* wk = reinterpret_cast<uint8_t*>(work);
    hipStream_t st = (hipStream_t)stream;
    jpeg_ent_layout_kernel<<<dim3(1), kG, 0, st>>>(dd, B, files_bytes, wk);
    MPN_LAUNCH_CHECK();
    jpeg_ent_init_kernel<<<dim3(kInitGroups, (unsigned)B), kG, 0, st>>>(files, files_bytes, dd, B, coefs, coef_bytes,
                                                                       reinterpret_cast<mpn_jpeg_desc*>(jpeg_descs_out), wk);
    MPN_LAUNCH_CHECK();
    for (int pass = 1; pass <= max_passes; ++pass) {
        jpeg_ent_sync_kernel<<<dim3(kSyncGroups, (unsigned)B), kG, 0, st>>>(files, files_bytes, dd, B, coef_bytes, wk, pass);
        MPN_LAUNCH_CHECK();
    }
    jpeg_ent_prefix_kernel<<<dim3((unsigned)B), kG, 0, st>>>(files, files_bytes, dd, B, coef_bytes, wk, max_passes);
    MPN_LAUNCH_CHECK();
    jpeg_ent_write_kernel<<<dim3(kWriteGroups, (unsigned)B), kG, 0, st>>>(files, files_bytes, dd, B, coefs, coef_bytes, wk);
    MPN_LAUNCH_CHECK();
    jpeg_ent_dc_kernel<<<dim3(3, (unsigned)B), kG, 0, st>>>(files, files_bytes, dd, B, coefs, coef_bytes, wk,
                                                           reinterpret_cast<mpn_jpeg_entropy_record*>(records));
    MPN_LAUNCH_CHECK();
    return MPN_OK;
}
