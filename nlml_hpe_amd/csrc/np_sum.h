// np_sum.h -- numpy's pairwise np.sum over contiguous f64 (pairwise_sum_DOUBLE, numpy/_core/src/umath/loops_utils.h.src), written once
// for everything here that has to return np.sum's bits: the centroid normalisation (centroid_ref.h, normalize_centroid.hip: 468
// squared norms) and the Tucker objective and gradient in the reference's order (tucker_ref.h, tucker_gradient.hip, tucker_grad_ref.h:
// 1,404 residual products).  Plain C++ for the host and for device code.
//
//   n < 8          the elements added in sequence
//   8 <= n <= 128  a LEAF: eight accumulators seeded from the first eight elements, stride 8, combined
//                  ((r0+r1)+(r2+r3)) + ((r4+r5)+(r6+r7)), then the n % 8 remainder elements in sequence
//   n > 128        sum(a, h) + sum(a + h, n - h), h = n / 2 rounded down to a multiple of 8
//
// So a row of N elements is a binary tree of leaves that depends on N alone: NpTree<N> is that tree at compile time (a kernel gives its
// leaves to lanes), np_leaf_sum one leaf, np_tree_sum the levels above the leaves, np_pairwise_sum the recursion for any n on the host.
// Only additions, all with contraction off.
//
// NOT numpy's in one corner, on purpose: np.sum starts from +0.0, so a row of -0.0 values alone sums to +0.0 there and to -0.0 here
// (a leaf is seeded from its first elements).  No caller sums such a row (squares, and products of residuals that are not all -0.0), and
// the functions these replaced returned the same.
// (The C oracle keeps its own np_pairwise_sum, oracle/csrc/oracle.c: it is independent of this file on purpose.)
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NLML_NP_HD __host__ __device__
#else
#define NLML_NP_HD
#endif
#if defined(__clang__)
#define NLML_NP_STRICT _Pragma("clang fp contract(off)")
#else
#define NLML_NP_STRICT   // (additions only: nothing to contract)
#endif

namespace nlml {

constexpr int NP_LEAF_MAX = 128;   // numpy's PW_BLOCKSIZE: a longer range splits

// where numpy splits a range of n > 128 elements
constexpr int np_split(int n) { return n / 2 - (n / 2) % 8; }

// The tree of a row of N elements: `leaves`, and leaf L = elements [off(L), off(L) + len(L)); off(leaves) = N.  off and len are
// constexpr functions of selects over constants, so device code may call them with a run-time L.  `balanced`: every leaf at the same
// depth, i.e. the levels above the leaves are the balanced tree np_tree_sum<leaves> adds.
template <int N, bool IS_LEAF = (N <= NP_LEAF_MAX)>
struct NpTree;
template <int N>
struct NpTree<N, true> {
  static_assert(N >= 8, "a leaf has its eight accumulators");
  static constexpr int leaves = 1, depth = 0;
  static constexpr bool balanced = true;
  static constexpr int off(int L) { return L <= 0 ? 0 : N; }
  static constexpr int len(int L) { return off(L + 1) - off(L); }
};
template <int N>
struct NpTree<N, false> {
  typedef NpTree<np_split(N)> Lo;
  typedef NpTree<N - np_split(N)> Hi;
  static constexpr int leaves = Lo::leaves + Hi::leaves, depth = 1 + (Lo::depth > Hi::depth ? Lo::depth : Hi::depth);
  static constexpr bool balanced = Lo::balanced && Hi::balanced && Lo::depth == Hi::depth;
  static constexpr int off(int L) { return L < Lo::leaves ? Lo::off(L) : np_split(N) + Hi::off(L - Lo::leaves); }
  static constexpr int len(int L) { return off(L + 1) - off(L); }
};

// the two trees the kernels are laid out for
constexpr bool np_tree_1404_is(int L = 0) {   // 16 leaves of 80, 14 x 88, 92, starting at 80 + 88 (L - 1)
  return L == 16 ? NpTree<1404>::off(16) == 1404
                 : NpTree<1404>::off(L) == (L == 0 ? 0 : 80 + 88 * (L - 1)) && NpTree<1404>::len(L) == (L == 0 ? 80 : L == 15 ? 92 : 88) &&
                       np_tree_1404_is(L + 1);
}
static_assert(NpTree<468>::leaves == 4 && NpTree<468>::balanced, "468 -> 232 + 236 -> (112 + 120) + (112 + 124)");
static_assert(NpTree<468>::off(1) == 112 && NpTree<468>::off(2) == 232 && NpTree<468>::off(3) == 344 && NpTree<468>::off(4) == 468, "468: offsets");
static_assert(NpTree<468>::len(0) == 112 && NpTree<468>::len(1) == 120 && NpTree<468>::len(2) == 112 && NpTree<468>::len(3) == 124, "468: lengths");
static_assert(NpTree<1404>::leaves == 16 && NpTree<1404>::balanced && np_tree_1404_is(), "1404 -> 16 leaves: 80, 14 x 88, 92");

// one leaf, 8 <= n <= 128 (P: a pointer to double in any address space)
template <typename P>
NLML_NP_HD inline double np_leaf_sum(P a, int n) {
  NLML_NP_STRICT
  double r0 = a[0], r1 = a[1], r2 = a[2], r3 = a[3], r4 = a[4], r5 = a[5], r6 = a[6], r7 = a[7];
  int i = 8;
  for (; i < n - (n % 8); i += 8) {
    r0 += a[i + 0]; r1 += a[i + 1]; r2 += a[i + 2]; r3 += a[i + 3];
    r4 += a[i + 4]; r5 += a[i + 5]; r6 += a[i + 6]; r7 += a[i + 7];
  }
  double res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
  for (; i < n; ++i) res += a[i];
  return res;
}

// the levels above the leaves of a balanced tree: (leaf[0] + leaf[1]) + (leaf[2] + leaf[3]) for four, the same over the four quarters'
// sums for sixteen.  A caller asserts NpTree<N>::balanced for its N.  (Taken by quarters and not by halves: the same tree, and the
// order in which the kernels have always written its additions down.)
template <int LEAVES, typename P>
NLML_NP_HD inline double np_tree_sum(P leaf) {
  NLML_NP_STRICT
  static_assert(LEAVES >= 1 && (LEAVES & (LEAVES - 1)) == 0, "a balanced tree has 2^k leaves");
  if constexpr (LEAVES == 1) {
    return leaf[0];
  } else if constexpr (LEAVES == 2) {
    return leaf[0] + leaf[1];
  } else {
    constexpr int Q = LEAVES / 4;
    const double a0 = np_tree_sum<Q>(leaf), a1 = np_tree_sum<Q>(leaf + Q), a2 = np_tree_sum<Q>(leaf + 2 * Q), a3 = np_tree_sum<Q>(leaf + 3 * Q);
    return (a0 + a1) + (a2 + a3);
  }
}

// np.sum of n contiguous doubles, any n >= 0 (host: the recursion is a real one)
inline double np_pairwise_sum(const double* a, int n) {
  NLML_NP_STRICT
  if (n < 8) {
    double res = 0.0;
    for (int i = 0; i < n; ++i) res += a[i];
    return res;
  }
  if (n <= NP_LEAF_MAX) return np_leaf_sum(a, n);
  const int h = np_split(n);
  return np_pairwise_sum(a, h) + np_pairwise_sum(a + h, n - h);
}

}  // namespace nlml
