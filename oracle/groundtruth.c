/* GROUND TRUTH — TEST INFRASTRUCTURE ONLY (tests/test_ground_truth.py, tests/matrixtruth.py).
 *
 * NOT a restatement of the reference: textbook dynamic programming that knows nothing about search schemes, FM
 * indexes, bit-parallel matrices or the oracle.  It answers two questions about a reported occurrence list that
 * neither the oracle (oracle_search.hpp, the builder's reading of the reference) nor the HIP path can answer about
 * themselves:
 *   soundness     is the distance reported for text[begin, end) an edit / Hamming distance that this text window
 *                 really has to the read?                                          -> gt_edit_distance
 *   completeness  which end positions of the text are within k edits of the read at all (Sellers' semi-global
 *                 alignment, free start in the text)?                              -> gt_semiglobal_ends
 * Further down, for tests/matrixtruth.py: a full integer matrix with a given first column and what follows from it cell by cell
 * (row verdicts, rightmost active columns, tracebacks, match words) — what the bit-parallel matrices must compute.
 * Alphabet handling follows the matcher's contract (reads.h:43-58, alphabet.h:52-64 of the reference): the caller
 * hands over read characters already upper-cased with everything outside ACGT replaced by 'N'; an 'N' in the read
 * matches nothing, and neither does a text character outside ACGT.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static inline int eq(uint8_t p, uint8_t t) {
    return p == t && (p == 'A' || p == 'C' || p == 'G' || p == 'T');
}

/* plain O(la * lb) edit distance of pattern a against text window b (unit costs) */
uint32_t gt_edit_distance(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
    uint32_t* prev = (uint32_t*)malloc((size_t)(lb + 1) * sizeof(uint32_t));
    uint32_t* cur = (uint32_t*)malloc((size_t)(lb + 1) * sizeof(uint32_t));
    for (uint32_t j = 0; j <= lb; j++) prev[j] = j;
    for (uint32_t i = 1; i <= la; i++) {
        cur[0] = i;
        for (uint32_t j = 1; j <= lb; j++) {
            uint32_t d = prev[j - 1] + (eq(a[i - 1], b[j - 1]) ? 0u : 1u);
            const uint32_t u = prev[j] + 1, l = cur[j - 1] + 1;
            if (u < d) d = u;
            if (l < d) d = l;
            cur[j] = d;
        }
        uint32_t* t = prev;
        prev = cur;
        cur = t;
    }
    const uint32_t r = prev[lb];
    free(prev);
    free(cur);
    return r;
}

uint32_t gt_hamming_distance(const uint8_t* a, const uint8_t* b, uint32_t l) {
    uint32_t d = 0;
    for (uint32_t i = 0; i < l; i++) d += eq(a[i], b[i]) ? 0u : 1u;
    return d;
}

/* Sellers: best[j] = min over b <= j of the edit distance between the pattern and text[b, j), for every end position
 * j = 0 .. n, capped at k + 1.  Column-wise with Ukkonen's cut-off (only the cells <= k of a column are kept), which
 * is exact for all values <= k.  Also returns, per end position with best[j] <= k, the LARGEST begin position of an
 * optimal alignment ending there (begin[j]; the shortest optimal window), else 0. */
void gt_semiglobal_ends(const uint8_t* text, uint64_t n, const uint8_t* pat, uint32_t m, uint32_t k, uint8_t* best,
                        uint64_t* begin) {
    const uint32_t INF = k + 1;
    uint32_t* col = (uint32_t*)malloc((size_t)(m + 1) * sizeof(uint32_t));
    uint64_t* org = (uint64_t*)malloc((size_t)(m + 1) * sizeof(uint64_t)); /* begin of the best alignment of the cell */
    for (uint32_t i = 0; i <= m; i++) {
        col[i] = i <= k ? i : INF;
        org[i] = 0;
    }
    uint32_t last = k < m ? k : m; /* last row whose value is <= k */
    best[0] = (uint8_t)(m <= k ? m : INF);
    if (begin) begin[0] = 0;
    for (uint64_t j = 1; j <= n; j++) {
        const uint8_t t = text[j - 1];
        uint32_t diag = col[0];
        uint64_t diagOrg = org[0];
        col[0] = 0;
        org[0] = j; /* an alignment may start right here */
        const uint32_t upto = last + 1 < m ? last + 1 : m;
        for (uint32_t i = 1; i <= upto; i++) {
            const uint32_t oldV = col[i];
            const uint64_t oldO = org[i];
            /* diagonal (match / substitution), vertical in this column (pattern char unmatched), horizontal (text char
             * unmatched: from the previous column's same row = oldV) */
            uint32_t d = diag + (eq(pat[i - 1], t) ? 0u : 1u);
            uint64_t o = diagOrg;
            const uint32_t v = col[i - 1] + 1;
            if (v < d || (v == d && org[i - 1] > o)) {
                d = v;
                o = org[i - 1];
            }
            const uint32_t h = (i <= last ? oldV : INF) + 1;
            if (h < d || (h == d && oldO > o && i <= last)) {
                d = h;
                o = oldO;
            }
            if (d > INF) d = INF;
            col[i] = d;
            org[i] = o;
            diag = i <= last ? oldV : INF;
            diagOrg = oldO;
        }
        last = upto;
        while (last > 0 && col[last] > k) last--;
        if (last == m) {
            best[j] = (uint8_t)col[m];
            if (begin) begin[j] = org[m];
        } else {
            best[j] = (uint8_t)INF;
            if (begin) begin[j] = 0;
        }
    }
    free(col);
    free(org);
}

/* ---- cell-level truth for the bit-parallel matrices (tests/matrixtruth.py) ----
 * A full, unbanded integer matrix with a given first column: D[i][0] = initED[i] for i < nInit, then +1 per row;
 * D[0][j] = initED[0] + j; the usual recurrence elsewhere.  X runs along the columns, Y along the rows; columns beyond X
 * (the band may reach past the last one) match nothing.  Everything below is derived from these integers alone. */
static uint32_t* gt_full_matrix(const uint8_t* X, uint32_t xLen, const uint8_t* Y, uint32_t rows, const uint32_t* initED,
                                uint32_t nInit, uint32_t cols) {
    uint32_t* D = (uint32_t*)malloc((size_t)(rows + 1) * cols * sizeof(uint32_t));
    for (uint32_t j = 0; j < cols; j++) D[j] = initED[0] + j;
    for (uint32_t i = 1; i <= rows; i++) {
        uint32_t* r = D + (size_t)i * cols;
        const uint32_t* p = r - cols;
        r[0] = i < nInit ? initED[i] : p[0] + 1;
        for (uint32_t j = 1; j < cols; j++) {
            uint32_t d = p[j - 1] + ((j <= xLen && eq(X[j - 1], Y[i - 1])) ? 0u : 1u);
            if (p[j] + 1 < d) d = p[j] + 1;
            if (r[j - 1] + 1 < d) d = r[j - 1] + 1;
            r[j] = d;
        }
    }
    return D;
}

typedef struct {
    uint32_t n, m, Wv, Wh, rows, cols;
} gt_geom;
static gt_geom gt_geometry(uint32_t xLen, uint32_t yLen, const uint32_t* initED, uint32_t nInit, uint32_t maxED) {
    gt_geom g;
    g.n = xLen + 1;
    g.Wv = nInit - 1 + maxED - initED[nInit - 1];
    g.Wh = maxED - initED[0];
    g.m = g.Wv + g.n;
    if (g.Wv + g.Wh + 1 > g.m) g.m = g.Wv + g.Wh + 1;
    g.rows = yLen < g.m - 1 ? yLen : g.m - 1;
    g.cols = g.n + g.Wh + 2 > g.rows + g.Wh + 2 ? g.n + g.Wh + 2 : g.rows + g.Wh + 2;
    return g;
}

/* The first column continues to the left of column 0: the reference keeps the first-column values of the rows below row i on row i's
 * own diagonals, so cell (i, -t) is the first-column value of row i + t (bitparallelmatrix.cpp:105-121). */
static uint32_t gt_cell(const uint32_t* D, uint32_t cols, uint32_t i, int32_t j, const uint32_t* initED, uint32_t nInit) {
    if (j >= 0) return D[(size_t)i * cols + (uint32_t)j];
    const uint32_t r = i + (uint32_t)(-j);
    return r < nInit ? initED[r] : initED[nInit - 1] + (r - nInit + 1);
}

/* The rightmost active column of row i from that of row i - 1 (bitparallelmatrix.h:398-412 on integers): one column to the right
 * if the diagonal step into it costs nothing; otherwise the rightmost column at or left of it, not left of i - Wv, whose cell is
 * at most maxED; INT32_MIN if there is none (the row is invalid).  *event: 2 = moved by the diagonal rule, 1 = a negative horizontal
 * step lies between the column the walk starts at and the column it ends at (the general walk). */
#define GT_NO_RAC INT32_MIN
static int32_t gt_next_rac(const uint32_t* D, uint32_t cols, uint32_t i, int32_t rac, uint32_t Wv, uint32_t maxED, const uint32_t* initED,
                           uint32_t nInit, uint8_t* event) {
    const int32_t c = rac + 1;
    *event = 0;
    if (gt_cell(D, cols, i, c, initED, nInit) == gt_cell(D, cols, i - 1, rac, initED, nInit)) {
        *event = 2;
        return c;
    }
    const int32_t stop = (int32_t)i - (int32_t)Wv;
    for (int32_t j = c; j >= stop; j--)
        if (gt_cell(D, cols, i, j, initED, nInit) <= maxED) {
            for (int32_t cc = j + 1; cc <= c; cc++)
                if (gt_cell(D, cols, i, cc, initED, nInit) + 1 == gt_cell(D, cols, i, cc - 1, initED, nInit)) *event = 1;
            return j;
        }
    return GT_NO_RAC;
}

/* Rows 1 .. min(yLen, m - 1) of one case, up to and including its first invalid row.  Per row: verdict (1 valid), the rightmost
 * active column (INT32_MIN on an invalid row), the event bits of gt_next_rac, the first column of the band and the cells of columns
 * firstColumn(i) .. min(n - 1, i + Wh), saturated at 255, `stride` bytes per row.  Returns the number of rows written. */
uint32_t gt_matrix_rows(const uint8_t* X, uint32_t xLen, const uint8_t* Y, uint32_t yLen, const uint32_t* initED, uint32_t nInit,
                        uint32_t maxED, uint32_t stride, uint8_t* verdict, int32_t* racOut, uint8_t* events, uint32_t* firstCol,
                        uint32_t* nCells, uint8_t* cells) {
    const gt_geom g = gt_geometry(xLen, yLen, initED, nInit, maxED);
    uint32_t* D = gt_full_matrix(X, xLen, Y, g.rows, initED, nInit, g.cols);
    int32_t rac = (int32_t)g.Wh;
    uint32_t i = 1;
    for (; i <= g.rows; i++) {
        const uint32_t* r = D + (size_t)i * g.cols;
        rac = gt_next_rac(D, g.cols, i, rac, g.Wv, maxED, initED, nInit, &events[i - 1]);
        verdict[i - 1] = rac != GT_NO_RAC;
        racOut[i - 1] = rac;
        const uint32_t fc = i <= g.Wv ? 0u : i - g.Wv;
        const uint32_t lc = g.n - 1 < i + g.Wh ? g.n - 1 : i + g.Wh;
        firstCol[i - 1] = fc;
        uint32_t nc = 0;
        for (uint32_t j = fc; j <= lc && nc < stride; j++) cells[(size_t)(i - 1) * stride + nc++] = (uint8_t)(r[j] > 255 ? 255 : r[j]);
        nCells[i - 1] = nc;
        if (rac == GT_NO_RAC) {
            i++;
            break;
        }
    }
    free(D);
    return i - 1;
}

/* The tracebacks of one in-text case (first column: nZeros zeros): from (i, n - 1) for every valid final-column row i whose
 * cell is at most maxED, to column 0 — horizontal if D[i][j] == D[i][j-1] + 1, else diagonal if the characters match or
 * D[i][j] == D[i-1][j-1] + 1, else vertical; row 0 steps horizontally only.  Per walk `recWords` 16-bit words: start row, the row
 * reached at column 0, number of runs, 0, then the runs (length << 2 | op; op 0 = diagonal, 1 = horizontal, 2 = vertical) in
 * walk order.  With rel = j + below - i, strata[0] counts steps at rel <= relLo, strata[1] steps at rel >= relHi that are not
 * horizontal (narrow rows) or any step there (relHiAny), strata[2] walks that visit two groups of `groupRows` stored rows,
 * strata[3] walks that end in row 0; strata[4] is set to the number of valid rows.  Returns the number of walks (at most maxWalks). */
uint32_t gt_trace_walks(const uint8_t* X, uint32_t xLen, const uint8_t* Y, uint32_t yLen, uint32_t nZeros, uint32_t maxED,
                        uint32_t below, uint32_t relLo, uint32_t relHi, uint32_t relHiAny, uint32_t groupRows, uint32_t recWords,
                        uint32_t maxWalks, uint16_t* out, uint64_t* strata) {
    uint32_t initED[64];
    for (uint32_t i = 0; i < nZeros; i++) initED[i] = 0;
    const gt_geom g = gt_geometry(xLen, yLen, initED, nZeros, maxED);
    uint32_t* D = gt_full_matrix(X, xLen, Y, g.rows, initED, nZeros, g.cols);
    int32_t rac = (int32_t)g.Wh;
    uint32_t valid = 0;
    for (uint32_t i = 1; i <= g.rows; i++) {
        uint8_t ev;
        rac = gt_next_rac(D, g.cols, i, rac, g.Wv, maxED, initED, nZeros, &ev);
        if (rac == GT_NO_RAC) break;
        valid = i;
    }
    const uint32_t sfc = g.Wh + g.Wv + 1, col = g.n - 1;
    uint32_t nWalks = 0;
    strata[4] = valid;
    for (uint32_t s = g.m - sfc; s <= valid && nWalks < maxWalks; s++) {
        if (D[(size_t)s * g.cols + col] > maxED) continue;
        uint16_t* rec = out + (size_t)nWalks * recWords;
        uint32_t ti = s, tj = col, nRuns = 0, state = 3, run = 0;
        while (tj > 0) {
            const uint32_t* r = D + (size_t)ti * g.cols;
            const uint32_t rel = tj + below - ti;
            uint32_t op;
            if (r[tj] == r[tj - 1] + 1) op = 1;
            else if (ti > 0 && (eq(X[tj - 1], Y[ti - 1]) || r[tj] == (r - g.cols)[tj - 1] + 1)) op = 0;
            else op = 2;
            if (rel <= relLo) strata[0]++;
            if (rel >= relHi && (relHiAny || op != 1)) strata[1]++;
            if (op != state) {
                if (run) {
                    if (4 + nRuns < recWords) rec[4 + nRuns] = (uint16_t)((run << 2) | state);
                    nRuns++;
                }
                state = op;
                run = 0;
            }
            run++;
            if (op == 1) tj--;
            else if (op == 0) ti--, tj--;
            else ti--;
        }
        if (run) {
            if (4 + nRuns < recWords) rec[4 + nRuns] = (uint16_t)((run << 2) | state);
            nRuns++;
        }
        rec[0] = (uint16_t)s;
        rec[1] = (uint16_t)ti;
        rec[2] = (uint16_t)nRuns;
        rec[3] = 0;
        if ((s - 1) / groupRows != ((ti ? ti : 1) - 1) / groupRows) strata[2]++;
        if (ti == 0) strata[3]++;
        nWalks++;
    }
    free(D);
    return nWalks;
}

/* The match word of block b of a matrix with `left` margin bits and `block` rows per block, for nucleotide ch, as a character
 * comparison: bit t stands for character t - left + block * b of X; one to the left of X, zero beyond it. */
uint64_t gt_match_word(const uint8_t* X, uint32_t xLen, uint32_t left, uint32_t block, uint32_t b, uint8_t ch) {
    uint64_t w = 0;
    for (uint32_t t = 0; t < 64; t++) {
        const int64_t j = (int64_t)t - (int64_t)left + (int64_t)block * b;
        if (j < 0 || (j < (int64_t)xLen && eq(X[j], ch))) w |= 1ull << t;
    }
    return w;
}

/* n match words at once: X of query q is pool[xStart[q] .. xStart[q] + xLen[q]) */
void gt_match_words(const uint8_t* pool, const uint32_t* xStart, const uint32_t* xLen, const uint32_t* left, const uint32_t* block,
                    const uint32_t* b, const uint8_t* ch, uint64_t n, uint64_t* out) {
    for (uint64_t q = 0; q < n; q++) out[q] = gt_match_word(pool + xStart[q], xLen[q], left[q], block[q], b[q], ch[q]);
}
