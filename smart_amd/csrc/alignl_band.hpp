// alignl_band.hpp — byte texts, LONG patterns: start position and alignment of ONE edit-distance occurrence
// (smartgpu_align_editl64, talignl.hpp) as a BAND of the reversed matrix of edit_align.hpp,
//     D'[i][j] = ed(P[m-i .. m), T[e-j+1 .. e]),   D'[0][j] = j,  D'[i][0] = i,   0 <= i <= m, 0 <= j <= ncols,
// computed anti-diagonal by anti-diagonal with ONE LANE PER DIAGONAL: lane l of 64 owns d = j - i = l - 32 and is live when
// |d| <= k <= 31.  What is here is what a lane decides by itself — which cell it computes at step a, the cell's value and the
// operation the traceback would take there, where that operation is kept, how the lanes' last values become (distance, J),
// and where operation t of the alignment goes.  How a lane gets its neighbours' values is the caller's: text_editl_align
// (k_talignl.hip) by wave shifts, tests/text_alignl_check.cpp from an array of 64 lanes.  Host and device, no HIP call, no
// other header of the library but talign_host.hpp (the window's geometry) and edit_align.hpp (the operations' codes).
//
// WHY THE BAND IS EXACT.  A dead lane and a lane that has not started count as kAlignlBig.  (1) Band values >= true values:
// every band cell is a minimum over a subset of the true cell's candidates, each >= its true value by induction.
// (2) D'[i][j] >= |i - j|: a path to (i, j) takes at least |i - j| steps off the diagonal.  (3) A cell with true value
// v <= k has an optimal predecessor with true value <= v <= k, which by (2) lies on a live diagonal and by induction holds
// its true value in the band: so the band holds v.  Together: every cell whose true value is <= k is exact, every other
// band value is > k.  The minimum of row m over the band is therefore D(e) when D(e) <= k and > k otherwise, and the
// columns that reach it are the true ones.
//
// WHY DECIDING AT COMPUTE TIME EQUALS DECIDING DURING THE WALK.  edit_traceback (edit_align.hpp) asks at a cell of the path,
// whose value cur <= k is exact: diag + miss == cur, else up + 1 == cur, else 'I'.  alignl_cell asks the same of the band
// values.  A candidate whose TRUE value meets cur is <= k, hence exact in the band, and the test holds there too; a
// candidate whose true value exceeds it is no smaller in the band by (1), and the test fails there too.  So the two bits a
// lane stores when it computes the cell are the walk's choice, and the walk only ever reads cells of value <= k.
#pragma once
#include "edit_align.hpp"
#include "talign_host.hpp"

namespace sg {

constexpr uint32_t kAlignlMaxM = 256;   // SMARTGPU_EDITL_MAXM
constexpr uint32_t kAlignlMaxK = 31;    // SMARTGPU_EDITL_MAXK
constexpr uint32_t kAlignlLanes = 64;   // one wave: the diagonals -32 .. 31, of which -k .. k are live
constexpr int kAlignlMid = 32;          // the lane of diagonal 0
constexpr int kAlignlBig = 0x3fff;      // a dead or not-yet-started neighbour: above every distance, far below overflow
constexpr uint32_t kAlignlMaxOps = kAlignlMaxM + kAlignlMaxK;    // 287: the longest alignment
constexpr uint32_t kAlignlOpsWords = 10;                         // SMARTGPU_ALIGNL_OPS_WORDS: nine of operations, one of L
constexpr uint32_t kAlignlDecRows = 16;                          // rows of decisions in a dword
constexpr uint32_t kAlignlDecDw = kAlignlMaxM / kAlignlDecRows + 1;  // 17 dwords per lane: [row / 16][lane], rows 0 .. 256
// the window: the ALIGNED dwords ending at text dword e >> 2 that hold m + k <= 287 bytes ending anywhere in a dword
constexpr uint32_t kAlignlWinDw = 1u + (kAlignlMaxOps - 1u + 3u) / 4u;
static_assert(kAlignlMaxK < kAlignlMid && kAlignlMid + (int)kAlignlMaxK < (int)kAlignlLanes, "every live diagonal has a lane");
static_assert(kAlignlMaxOps == 287 && (kAlignlOpsWords - 1) * 32 >= kAlignlMaxOps, "nine words hold the longest alignment");
static_assert(kAlignlDecDw == 17, "sixteen rows per dword, rows 0 .. 256");
static_assert(kAlignlWinDw == 73 && 4 * (kAlignlWinDw - 1) + 1 >= kAlignlMaxOps && 4 * (kAlignlWinDw - 2) + 1 < kAlignlMaxOps,
              "the window holds the longest walk at e % 4 == 0, and not a dword more");
static_assert(kAlignlWinDw <= 2 * kAlignlLanes, "a wave loads its window with two loads per lane");

// the diagonal of a lane, and whether it takes part for this k
SG_HOST_DEVICE inline int alignl_diag(uint32_t lane) { return static_cast<int>(lane) - kAlignlMid; }
SG_HOST_DEVICE inline bool alignl_live(int d, uint32_t k) { return d >= -static_cast<int>(k) && d <= static_cast<int>(k); }

// The cell a lane of diagonal d computes at step a = i + j (0 <= a <= m + ncols), if any: a and d of one parity, and the
// cell inside the matrix.  The cell (i-1, j) is lane d + 1's of step a - 1, (i, j-1) lane d - 1's of step a - 1, (i-1, j-1)
// the lane's own of step a - 2: a lane needs its neighbours' LATEST values and its own, nothing older.
SG_HOST_DEVICE inline bool alignl_step_cell(uint32_t a, int d, uint32_t m, uint32_t ncols, uint32_t* i, uint32_t* j)
{
    const int lo = static_cast<int>(a) - d, hi = static_cast<int>(a) + d;
    *i = static_cast<uint32_t>(lo) >> 1;
    *j = static_cast<uint32_t>(hi) >> 1;
    return lo >= 0 && hi >= 0 && !(lo & 1) && *i <= m && *j <= ncols;
}

// An interior cell (i, j >= 1): its value and the operation edit_traceback would take there — the diagonal first ('=' or
// 'X'), then 'D' (the pattern symbol alone: up), then 'I' (the text symbol alone: left).
struct AlignlCell {
    int value;
    uint32_t op;
};
SG_HOST_DEVICE inline AlignlCell alignl_cell(int diag, int up, int left, uint32_t miss)
{
    const int dv = diag + static_cast<int>(miss), uv = up + 1, lv = left + 1;
    const int side = uv < lv ? uv : lv;
    AlignlCell c;
    c.value = dv < side ? dv : side;
    c.op = dv == c.value ? (miss ? kOpSub : kOpEq) : uv == c.value ? kOpDel : kOpIns;
    return c;
}

// miss of cell (i, j), i >= 1: bit (i - 1) % 32 of dword (i - 1) / 32 of the byte's mask of the REVERSED pattern, in the
// word-major table of teditl_host.hpp (table[w * 256 + byte]); alignl_peq_index is the dword to read
SG_HOST_DEVICE inline uint32_t alignl_peq_index(uint32_t i, uint32_t byte) { return ((i - 1u) >> 5) * 256u + byte; }
SG_HOST_DEVICE inline uint32_t alignl_miss(uint32_t i, uint32_t peq_dword) { return ((peq_dword >> ((i - 1u) & 31u)) & 1u) ^ 1u; }

// Where the decision of cell (i, j) is kept: dword dec[alignl_dec_dword(i) * kAlignlLanes + lane of j - i], two bits at
// alignl_dec_shift(i).  A lane gathers sixteen rows in a register and stores the dword when alignl_dec_flush says so: at
// the last row of a dword and at the lane's last cell (row m, or column ncols).
SG_HOST_DEVICE inline uint32_t alignl_dec_dword(uint32_t i) { return i / kAlignlDecRows; }
SG_HOST_DEVICE inline uint32_t alignl_dec_shift(uint32_t i) { return 2u * (i % kAlignlDecRows); }
SG_HOST_DEVICE inline bool alignl_dec_flush(uint32_t i, uint32_t j, uint32_t m, uint32_t ncols)
{
    return i % kAlignlDecRows == kAlignlDecRows - 1 || i == m || j == ncols;
}
// (the lane of a cell of the band; masked, so that a walk over decisions that no hit can hold still reads inside the region)
SG_HOST_DEVICE inline uint32_t alignl_dec_lane(uint32_t i, uint32_t j)
{
    return static_cast<uint32_t>(static_cast<int>(j) - static_cast<int>(i) + kAlignlMid) & (kAlignlLanes - 1u);
}

// A lane's value at row m, D'[m][j], as a key whose minimum over the wave is the smallest distance and, among equal
// distances, the smallest j (the largest nearest start); a lane that never reached row m passes kAlignlKeyNone
constexpr uint32_t kAlignlKeyShift = 9;  // j <= 287 < 512
SG_HOST_DEVICE inline uint32_t alignl_key(int value, uint32_t j) { return static_cast<uint32_t>(value) << kAlignlKeyShift | j; }
constexpr uint32_t kAlignlKeyNone = static_cast<uint32_t>(kAlignlBig) << kAlignlKeyShift | ((1u << kAlignlKeyShift) - 1u);
SG_HOST_DEVICE inline uint32_t alignl_key_dist(uint32_t key) { return key >> kAlignlKeyShift; }
SG_HOST_DEVICE inline uint32_t alignl_key_j(uint32_t key) { return key & ((1u << kAlignlKeyShift) - 1u); }

// Operation t of the alignment (text order: the walk from (m, J) to (0, 0)): bits 2 * (t % 32) of word t / 32, words 0 .. 8;
// word 9 is the length L.  On the device lane t / 32 ORs into its own word.
SG_HOST_DEVICE inline uint32_t alignl_op_word(uint32_t t) { return t >> 5; }
SG_HOST_DEVICE inline unsigned long long alignl_op_bits(uint32_t t, uint32_t op) { return static_cast<unsigned long long>(op) << (2u * (t & 31u)); }

// One step of the walk at (i, j) != (0, 0): row 0 is 'I', column 0 is 'D', otherwise the stored decision `dec2` (two bits).
// Lowers i, j or both; returns the operation.
SG_HOST_DEVICE inline uint32_t alignl_walk_step(uint32_t* i, uint32_t* j, uint32_t dec2)
{
    const uint32_t op = *i == 0 ? kOpIns : *j == 0 ? kOpDel : dec2;
    if (op != kOpIns) --*i;
    if (op != kOpDel) --*j;
    return op;
}

}  // namespace sg
