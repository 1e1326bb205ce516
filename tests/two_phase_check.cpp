// Stand-alone host check of linear-programming_amd/csrc/two_phase_host.h (tests/test_two_phase_host.py compiles it
// with the host compiler and -fsanitize=address,undefined and runs it as a program): the rule of the step between the
// phases (src/simplex.lisp:405-434) with T = double, float and a small integer struct that brings its own zero test.
// Every check that fails prints a "FAIL" line; each group that ran prints "ran NAME"; the exit status is the number
// of failures (0: all held).
#include "../linear-programming_amd/csrc/two_phase_host.h"

#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

static int g_failed = 0;
#define CHECK(c)                                                      \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);       \
            ++g_failed;                                               \
        }                                                             \
    } while (0)

struct Int3 { long v; };                                   // "exact" numbers: no operator==, only its own zero test
static bool is_zero(const Int3 &x) { return x.v == 0; }
static bool is_zero(double x) { return x == 0.0; }
static bool is_zero(float x) { return x == 0.0f; }
struct Zero { template <class T> bool operator()(const T &x) const { return is_zero(x); } };

template <class T> T num(long k) { return (T)k; }
template <> Int3 num<Int3>(long k) { return Int3{k}; }
template <class T> T tiny() { return std::numeric_limits<T>::denorm_min(); }     // the smallest thing that is not zero
template <> Int3 tiny<Int3>() { return Int3{1}; }

// ---------------------------------------------------------------------------------------------- tp_feasible
template <class T> static void check_feasible(const char *name)
{
    const T inf = std::numeric_limits<T>::infinity(), nan = std::numeric_limits<T>::quiet_NaN();
    for (T thr : {(T)1024 * std::numeric_limits<T>::epsilon() / 2, (T)0, (T)3.5}) {
        const T beyond = std::nextafter(thr, inf);
        CHECK(tp_feasible<T>(thr, thr) && tp_feasible<T>(-thr, thr));              // exactly at the threshold
        CHECK(!tp_feasible<T>(beyond, thr) && !tp_feasible<T>(-beyond, thr));      // the next value beyond it
        CHECK(tp_feasible<T>((T)0, thr) && tp_feasible<T>(-(T)0, thr));            // both zeros
        CHECK(!tp_feasible<T>(nan, thr) && !tp_feasible<T>(-nan, thr));
        CHECK(!tp_feasible<T>(inf, thr) && !tp_feasible<T>(-inf, thr));
    }
    CHECK(!tp_feasible<T>((T)0, nan));                                             // (no threshold, nothing passes)
    printf("ran feasible-%s\n", name);
}

// ---------------------------------------------------------------------------------------------- tp_entering_column
template <class T> static int64_t brute(const std::vector<T> &row, int64_t nv, const std::vector<int64_t> &basis, int64_t m)
{
    for (int64_t j = 0; j < nv; ++j) {
        if (is_zero(row[(size_t)j])) continue;
        bool basic = false;
        for (int64_t k = 0; k < m; ++k) basic = basic || basis[(size_t)k] == j;
        if (!basic) return j;
    }
    return -1;
}

template <class T>
static void column_is(const std::vector<T> &row, int64_t nv, const std::vector<int64_t> &basis, int64_t m, int64_t want, int line)
{
    const int64_t got = tp_entering_column(row.data(), nv, basis.data(), m, Zero());
    if (got != want || brute(row, nv, basis, m) != want) {
        printf("FAIL %s:%d  entering column %lld, brute force %lld, expected %lld\n", __FILE__, line, (long long)got,
               (long long)brute(row, nv, basis, m), (long long)want);
        ++g_failed;
    }
}
#define COLUMN_IS(T, ...) column_is<T>(__VA_ARGS__, __LINE__)

template <class T> static void check_entering_column(const char *name)
{
    const T o = num<T>(0), x = num<T>(3), y = num<T>(-2), t = tiny<T>();
    // 6 main columns, 2 artificial ones, the RHS; non-zero entries outside the main columns never count
    COLUMN_IS(T, {o, x, o, y, o, o, x, x, x}, 6, {1, 7, 6}, 3, 3);                 // column 1 is basic: the next one
    COLUMN_IS(T, {o, x, o, y, o, o, x, x, x}, 6, {3, 1, 6}, 3, -1);                // only basic columns hold non-zeros
    COLUMN_IS(T, {o, x, o, y, o, t, x, x, x}, 6, {3, 1, 6}, 3, 5);                 // the smallest non-zero qualifies
    COLUMN_IS(T, {o, o, o, o, o, o, x, x, x}, 6, {0, 1, 2}, 3, -1);                // an all-zero main part
    COLUMN_IS(T, {x, x, x, x, x, x, x, x, x}, 6, {7, 6, 8}, 3, 0);                 // a basis of artificial indices only
    COLUMN_IS(T, {x, x, x, x, x, x, x, x, x}, 0, {7, 6, 8}, 3, -1);                // num_vars = 0
    COLUMN_IS(T, {o, o, y, x, x, x, x, x, x}, 6, {2, 3, 4}, 0, 2);                 // m = 0: nothing is basic
    COLUMN_IS(T, {o, o, y, x, x, x, x, x, x}, 6, {2, 3, 4}, 2, 4);                 // ... and only basis[0..m) counts
    COLUMN_IS(T, {x}, 1, {}, 0, 0);
    printf("ran entering-column-%s\n", name);
}

template <class T> static void check_entering_column_ieee(const char *name)
{
    const T o = 0, mz = -(T)0, nan = std::numeric_limits<T>::quiet_NaN(), den = std::numeric_limits<T>::denorm_min();
    COLUMN_IS(T, {o, mz, o, -den, 1, 1}, 4, {0, 5}, 2, 3);                         // a denormal is not zero, -0.0 is
    COLUMN_IS(T, {mz, mz, mz, mz, 1, 1}, 4, {4, 5}, 2, -1);
    COLUMN_IS(T, {o, mz, nan, 1, 1, 1}, 4, {3, 5}, 2, 2);                          // NaN /= 0
    COLUMN_IS(T, {o, mz, nan, 1, 1, 1}, 4, {3, 2}, 2, -1);                         // ... in a basic column: skipped
    printf("ran entering-column-ieee-%s\n", name);
}

// ---------------------------------------------------------------------------------------------- tp_drive_out
// A 4 x 8 "device" tableau (5 main columns, 2 artificial ones, the RHS) behind recording lambdas.  Rows 1 and 3 hold
// basic artificials.  Row 1 takes column 4 (its other non-zero main entry is in basic column 1).  Row 3 as uploaded has
// non-zeros in columns 1, 3, 4 only: once column 4 is basic nothing qualifies -- unless the pivot changed the row, as
// the pivot lambda does when `pivot_touches_row3` (column 2 becomes non-zero).
template <class T> struct Rig {
    std::vector<std::vector<T>> A;
    std::vector<int64_t> basis{1, 5, 3, 6};
    std::string log;
    int count = 0;
    bool pivot_touches_row3 = true;
    int fetch_error_at = -1, fetch_error = 0, pivot_error_at = -1, pivot_error = 0;
    Rig()
    {
        const T o = num<T>(0), x = num<T>(3), y = num<T>(-2);
        A = {{x, x, x, x, x, o, o, x}, {o, y, o, o, x, x, o, o}, {x, x, x, x, x, o, o, x}, {o, x, o, y, x, o, x, o}};
    }
    int run(int64_t m = 4)
    {
        return tp_drive_out<T>(
            m, 5, 7, basis.data(), Zero(),
            [&](int64_t i, std::vector<T> &row) {
                log += "F" + std::to_string(i) + " ";
                if (i == fetch_error_at) return fetch_error;
                row = A[(size_t)i];
                return (int)MI_OK;
            },
            [&](int64_t col, int64_t i) {
                log += "P" + std::to_string(col) + "," + std::to_string(i) + " ";
                if (i == pivot_error_at) return pivot_error;
                if (pivot_touches_row3) A[3][2] = tiny<T>();
                return (int)MI_OK;
            },
            [&] { log += "C "; ++count; });
    }
};
using Basis = std::vector<int64_t>;

template <class T> static void check_drive_out(const char *name)
{
    {   // the order of calls; row 3 is fetched AFTER the pivot of row 1 and against the updated basis
        Rig<T> r;
        CHECK(r.run() == MI_OK && r.log == "F1 P4,1 C F3 P2,3 C " && r.count == 2 && r.basis == Basis({1, 4, 3, 2}));
    }
    {   // nothing qualifies in the second artificial row: the first pivot stays made and counted
        Rig<T> r;
        r.pivot_touches_row3 = false;
        CHECK(r.run() == MI_ART_STUCK && r.log == "F1 P4,1 C F3 " && r.count == 1 && r.basis == Basis({1, 4, 3, 6}));
    }
    {   // its RHS is not an exact zero (the smallest non-zero there is): MI_ART_NONZERO before any column is looked for
        Rig<T> r;
        r.A[3][7] = tiny<T>();
        CHECK(r.run() == MI_ART_NONZERO && r.log == "F1 P4,1 C F3 " && r.count == 1 && r.basis == Basis({1, 4, 3, 6}));
    }
    {   // ... in the FIRST artificial row: nothing is made
        Rig<T> r;
        r.A[1][7] = num<T>(-1);
        CHECK(r.run() == MI_ART_NONZERO && r.log == "F1 " && r.count == 0 && r.basis == Basis({1, 5, 3, 6}));
    }
    {   // errors of the lambdas pass through as they are, the count kept
        Rig<T> r;
        r.fetch_error_at = 3, r.fetch_error = -2;
        CHECK(r.run() == -2 && r.log == "F1 P4,1 C F3 " && r.count == 1 && r.basis == Basis({1, 4, 3, 6}));
        Rig<T> p;
        p.pivot_error_at = 3, p.pivot_error = 9;
        CHECK(p.run() == 9 && p.log == "F1 P4,1 C F3 P2,3 " && p.count == 1 && p.basis == Basis({1, 4, 3, 6}));
        Rig<T> q;
        q.pivot_error_at = 1, q.pivot_error = -7;
        CHECK(q.run() == -7 && q.log == "F1 P4,1 " && q.count == 0 && q.basis == Basis({1, 5, 3, 6}));
    }
    {   // no artificial basic, m = 0, and rows beyond m: no call at all
        Rig<T> r;
        r.basis = {1, 0, 3, 4};
        CHECK(r.run() == MI_OK && r.log.empty() && r.count == 0);
        Rig<T> e;
        CHECK(e.run(0) == MI_OK && e.log.empty() && e.count == 0);
        Rig<T> h;
        CHECK(h.run(2) == MI_OK && h.log == "F1 P4,1 C " && h.count == 1 && h.basis == Basis({1, 4, 3, 6}));
    }
    printf("ran drive-out-%s\n", name);
}

int main()
{
    check_feasible<double>("double");
    check_feasible<float>("float");
    check_entering_column<double>("double");
    check_entering_column<float>("float");
    check_entering_column<Int3>("int");
    check_entering_column_ieee<double>("double");
    check_entering_column_ieee<float>("float");
    check_drive_out<double>("double");
    check_drive_out<float>("float");
    check_drive_out<Int3>("int");
    printf("%d failed\n", g_failed);
    return g_failed ? 1 : 0;
}
