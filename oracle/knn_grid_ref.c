/*
 * knn_grid_ref.c -- TEST INFRASTRUCTURE ONLY.  A second, fast CPU oracle for distCUDA2.
 *
 * Only tests/ load this; the product path never touches it.  It returns the value knn_ref.c
 * returns, bit for bit, at sizes where knn_ref.c's O(P^2) is too slow: for each query i the
 * multiset of the three smallest fmaf(dz, dz, fmaf(dx, dx, dy * dy)), d = candidate - query in
 * float32, over every j != i (by index), kept in a list initialised to FLT_MAX that a candidate
 * enters only when strictly smaller than an entry; result ((b0 + b1) + b2) / 3.0f.  It is written
 * from that definition (knn_ref.c's header), and its search shares nothing with knn.hip: no Morton
 * order, no 64-point leaves, no boxes of consecutive points -- uniform cell grids scanned in rings.
 *
 * Search.  The points are split into a few disjoint SETS by nested boxes: the box
 * [q25 - 2.5 IQR, q75 + 2.5 IQR] per axis (quartiles of a strided sample) takes the points
 * inside it as one set, the rest go through the same split again, at most kMaxSets times.  Far
 * outliers, or a sparse shell round a dense core, so land in sets of their own and do not stretch the
 * dense set's grid.  Which point lands in which set changes speed only: every query searches EVERY
 * set, with one shared best-three list, so every j != i is either evaluated or excluded by a bound.
 * Each set has a grid of cubic cells of edge h over its own bounding box (x fastest; h shrinks until
 * a point shares its cell with few others, under a cap on the cell count), points stored cell by cell.
 *
 * For one query and one set:
 *   (a) the whole set is skipped if third_best is below the squared distance from the query to the
 *       set's bounding box;
 *   (b) otherwise with c = the query's cell, each coordinate clamped into the grid, the cells at
 *       Chebyshev distance r = 0, 1, 2, ... from c are scanned, every point in them evaluated, and the
 *       scan stops after ring r >= 1 once third_best is below ((r - 0.01) h)^2, or when ring r has
 *       reached every face of the grid (every cell scanned).
 *
 * Why this is exact.  A candidate with float32 distance d changes the multiset only if
 * d < third_best, and third_best only decreases; so a point may be left out if its d is >= the
 * third_best at the time of the decision.
 *   - Ring bound.  A point not scanned after ring r lies in a cell whose index differs from c's by
 *     at least r + 1 on some axis.  On that axis the query lies in c's slab, or beyond the grid's face
 *     on c's side when its cell was clamped (every point of the set is inside the grid, so clamping
 *     only moves the query away from them); the point's slab begins r whole cells further.  Its true
 *     distance is thus at least r h.  Cell indices are floor((x - lo) / h) in double; the rounding of
 *     that quotient displaces a slab face by ~1e-13 cells, which the 0.01 covers many times over.
 *   - Box bound.  Every point of the set is inside its bounding box, computed exactly from the
 *     float32 coordinates; the gap arithmetic in double is good to ~1e-15, a 1e-12 factor covers it.
 *   - float32 rounding.  "below" is  third_best (1 + 1e-6) + 2^-146 < bound, in double.  d is the
 *     rounded value of T = dx^2 + dy^2 + dz^2 with dx, dy, dz each one float32 subtraction (relative
 *     error 2^-24, exact in the subnormal range) and three roundings, each monotone, each off by at
 *     most 2^-24 relative in the normal range or 2^-150 absolute in the subnormal range.  So
 *     d >= T_true (1 - 2^-21) - 3 * 2^-150, and T_true >= bound > third_best (1 + 1e-6) + 2^-146
 *     gives d > third_best.  Overflow needs nothing more: if T exceeds FLT_MAX, d is FLT_MAX or +inf,
 *     never below a third_best that is at most FLT_MAX.
 *   - Ties at a bound change nothing: an omitted point with d == third_best would not have entered
 *     (strict '>'), and among scanned points only the multiset matters, not the order.
 * Non-finite coordinates are rejected (return 1): no cell holds a NaN.  Those inputs stay with
 * knn_ref.c.
 *
 * Build: oracle/Makefile, same flags as knn_ref.c (-ffp-contract=off: only the explicit fmaf fuses).
 */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

enum { kMaxSets = 8, kSample = 16384, kMaxAxisCells = 1024, kSmallSet = 64 };
static const long long kMaxCells = 1ll << 23;  /* per set: 32 MiB of cell starts, 256 MiB at kMaxSets */
static const double kTargetShare = 8.0;        /* mean number of points sharing a point's cell */

typedef struct {
    float x, y, z;
    int32_t idx;
} GPoint;

typedef struct {
    double lo[3], hi[3]; /* bounding box of the set's points */
    double h;            /* cell edge */
    int n[3];            /* cells per axis */
    uint32_t* start;     /* n[0] n[1] n[2] + 1 offsets into pts */
    GPoint* pts;         /* the set's points, cell by cell */
    long long count;
} GSet;

static inline int below(float third_best, double bound2)
{
    return (double)third_best * (1.0 + 1e-6) + 0x1p-146 < bound2;
}

static inline int cell_of(const GSet* g, int a, double x)
{
    double c = floor((x - g->lo[a]) / g->h);
    if (!(c > 0.0)) return 0;
    if (c > (double)(g->n[a] - 1)) return g->n[a] - 1;
    return (int)c;
}

static inline void scan_cells(const GSet* g, long long first, long long last, const GPoint* q, float* best)
{
    const GPoint* p = g->pts + g->start[first];
    const GPoint* end = g->pts + g->start[last + 1];
    for (; p < end; p++) {
        if (p->idx == q->idx) continue;
        const float dx = p->x - q->x, dy = p->y - q->y, dz = p->z - q->z;
        float dist = fmaf(dz, dz, fmaf(dx, dx, dy * dy));
        for (int j = 0; j < 3; j++) {
            if (best[j] > dist) {
                const float t = best[j];
                best[j] = dist;
                dist = t;
            }
        }
    }
}

static void search_set(const GSet* g, const GPoint* q, float* best)
{
    const double qc[3] = {q->x, q->y, q->z};
    double box2 = 0.0;
    int c[3], rmax = 0;
    for (int a = 0; a < 3; a++) {
        const double gap = fmax(fmax(g->lo[a] - qc[a], qc[a] - g->hi[a]), 0.0);
        box2 += gap * gap;
        c[a] = cell_of(g, a, qc[a]);
        if (c[a] > rmax) rmax = c[a];
        if (g->n[a] - 1 - c[a] > rmax) rmax = g->n[a] - 1 - c[a];
    }
    if (below(best[2], box2 * (1.0 - 1e-12))) return;
    const int nx = g->n[0], ny = g->n[1], nz = g->n[2];
    for (int r = 0; r <= rmax; r++) {
        const int x0 = c[0] - r < 0 ? 0 : c[0] - r, x1 = c[0] + r > nx - 1 ? nx - 1 : c[0] + r;
        const int y0 = c[1] - r < 0 ? 0 : c[1] - r, y1 = c[1] + r > ny - 1 ? ny - 1 : c[1] + r;
        const int z0 = c[2] - r < 0 ? 0 : c[2] - r, z1 = c[2] + r > nz - 1 ? nz - 1 : c[2] + r;
        for (int z = z0; z <= z1; z++) {
            const int zface = z - c[2] == r || c[2] - z == r;
            for (int y = y0; y <= y1; y++) {
                const long long row = ((long long)z * ny + y) * nx;
                if (zface || y - c[1] == r || c[1] - y == r) {
                    scan_cells(g, row + x0, row + x1, q, best);
                } else {
                    if (c[0] - r >= 0) scan_cells(g, row + c[0] - r, row + c[0] - r, q, best);
                    if (c[0] + r <= nx - 1) scan_cells(g, row + c[0] + r, row + c[0] + r, q, best);
                }
            }
        }
        if (r >= 1) {
            const double reach = (r - 0.01) * g->h;
            if (below(best[2], reach * reach)) return;
        }
    }
}

static long long cells_at(const GSet* g, double h, int* n)
{
    long long total = 1;
    for (int a = 0; a < 3; a++) {
        const double k = floor((g->hi[a] - g->lo[a]) / h) + 1.0;
        if (!(k <= (double)kMaxAxisCells)) return -1;
        n[a] = (int)k;
        total *= n[a];
    }
    return total <= kMaxCells ? total : -1;
}

static inline long long cell_index(const GSet* g, const float* p)
{
    return ((long long)cell_of(g, 2, p[2]) * g->n[1] + cell_of(g, 1, p[1])) * g->n[0] + cell_of(g, 0, p[0]);
}

/* Fills g for the points members[0, count) of pts: box, cell size, cell starts, points by cell. */
static int build_set(GSet* g, const float* pts, const int32_t* members, long long count)
{
    g->count = count;
    for (int a = 0; a < 3; a++) g->lo[a] = g->hi[a] = pts[3ll * members[0] + a];
    for (long long k = 1; k < count; k++)
        for (int a = 0; a < 3; a++) {
            const double v = pts[3ll * members[k] + a];
            if (v < g->lo[a]) g->lo[a] = v;
            if (v > g->hi[a]) g->hi[a] = v;
        }
    double ext = 0.0;
    for (int a = 0; a < 3; a++) ext = fmax(ext, g->hi[a] - g->lo[a]);
    g->h = ext > 0.0 ? ext * (1.0 + 1e-9) : 1.0; /* one cell: a small set is scanned whole */
    const double per_axis = cbrt((double)count / 4.0); /* first try: about 4 points per cell of a filled cube */
    if (per_axis > 1.5) g->h = 1.5 * ext / per_axis;
    g->n[0] = g->n[1] = g->n[2] = 1;
    uint32_t* cnt = NULL;
    if (count > kSmallSet && ext > 0.0) {
        /* shrink h while a point still shares its cell with more than kTargetShare on average,
           the sharing still falls, and the finer grid stays under the caps */
        double share_before = (double)count;
        for (;;) {
            int n[3];
            const double h = g->h / 1.5;
            const long long total = cells_at(g, h, n);
            if (total < 0 || total > 64 * count) break;
            const GSet keep = *g;
            g->h = h;
            memcpy(g->n, n, sizeof n);
            uint32_t* c2 = calloc((size_t)total + 1, sizeof *c2);
            if (!c2) { free(cnt); return 2; }
            for (long long k = 0; k < count; k++) c2[cell_index(g, pts + 3ll * members[k])]++;
            double share = 0.0;
            for (long long i = 0; i < total; i++) share += (double)c2[i] * c2[i];
            share /= (double)count;
            if (cnt && share > 0.95 * share_before) { /* duplicates: finer cells no longer separate */
                free(c2);
                *g = keep;
                break;
            }
            free(cnt);
            cnt = c2;
            share_before = share;
            if (share <= kTargetShare) break;
        }
    }
    const long long total = (long long)g->n[0] * g->n[1] * g->n[2];
    if (!cnt) {
        cnt = calloc((size_t)total + 1, sizeof *cnt);
        if (!cnt) return 2;
        for (long long k = 0; k < count; k++) cnt[cell_index(g, pts + 3ll * members[k])]++;
    }
    uint32_t run = 0;
    for (long long i = 0; i <= total; i++) { /* counts -> exclusive starts */
        const uint32_t c = cnt[i];
        cnt[i] = run;
        run += c;
    }
    g->start = cnt;
    g->pts = malloc((size_t)count * sizeof *g->pts);
    uint32_t* fill = malloc((size_t)total * sizeof *fill);
    if (!g->pts || !fill) { free(fill); return 2; }
    memcpy(fill, cnt, (size_t)total * sizeof *fill);
    for (long long k = 0; k < count; k++) {
        const float* p = pts + 3ll * members[k];
        const GPoint gp = {p[0], p[1], p[2], members[k]};
        g->pts[fill[cell_index(g, p)]++] = gp;
    }
    free(fill);
    return 0;
}

static int cmp_float(const void* a, const void* b)
{
    const float x = *(const float*)a, y = *(const float*)b;
    return (x > y) - (x < y);
}

/* Moves the members inside the quartile box to the front; returns how many. */
static long long split_by_box(const float* pts, int32_t* members, long long count, float* sample)
{
    double lo[3], hi[3];
    const long long m = count < kSample ? count : kSample, stride = count / m;
    for (int a = 0; a < 3; a++) {
        for (long long k = 0; k < m; k++) sample[k] = pts[3ll * members[k * stride] + a];
        qsort(sample, (size_t)m, sizeof *sample, cmp_float);
        const double q25 = sample[m / 4], q75 = sample[(3 * m) / 4];
        lo[a] = q25 - 2.5 * (q75 - q25);
        hi[a] = q75 + 2.5 * (q75 - q25);
    }
    long long in = 0;
    for (long long k = 0; k < count; k++) {
        const float* p = pts + 3ll * members[k];
        int inside = 1;
        for (int a = 0; a < 3; a++) inside &= p[a] >= lo[a] && p[a] <= hi[a];
        if (inside) {
            const int32_t t = members[in];
            members[in++] = members[k];
            members[k] = t;
        }
    }
    return in;
}

/* out[i] for every i in [0, P).  Returns 0, or 1: a non-finite coordinate (or P >= 2^31), 2: out of memory. */
int oracle_knn_mean3_grid(const float* pts, long long P, float* out)
{
    if (P <= 0) return 0;
    if (P > INT32_MAX) return 1;
    for (long long k = 0; k < 3 * P; k++)
        if (!isfinite(pts[k])) return 1;
    GSet sets[kMaxSets];
    int nsets = 0, rc = 0;
    memset(sets, 0, sizeof sets);
    int32_t* members = malloc((size_t)P * sizeof *members);
    float* sample = malloc(kSample * sizeof *sample);
    if (!members || !sample) rc = 2;
    if (!rc) {
        for (long long k = 0; k < P; k++) members[k] = (int32_t)k;
        int32_t* rest = members;
        long long nrest = P;
        while (nrest > 0 && !rc) {
            long long take = nrest;
            if (nsets < kMaxSets - 1 && nrest > kSmallSet) {
                take = split_by_box(pts, rest, nrest, sample);
                if (take == 0) take = nrest;
            }
            rc = build_set(&sets[nsets++], pts, rest, take);
            rest += take;
            nrest -= take;
        }
    }
    free(members);
    free(sample);
    if (!rc) {
        for (int s = 0; s < nsets; s++) {
            const GSet* own = &sets[s];
#pragma omp parallel for schedule(dynamic, 256)
            for (long long k = 0; k < own->count; k++) {
                const GPoint* q = own->pts + k;
                float best[3] = {FLT_MAX, FLT_MAX, FLT_MAX};
                search_set(own, q, best); /* its own set first: a tight bound for the others */
                for (int t = 0; t < nsets; t++)
                    if (t != s) search_set(&sets[t], q, best);
                out[q->idx] = (best[0] + best[1] + best[2]) / 3.0f;
            }
        }
    }
    for (int s = 0; s < nsets; s++) {
        free(sets[s].start);
        free(sets[s].pts);
    }
    return rc;
}
