// Stand-in for the part of glm the reference's CUDA files use. THE PROJECT'S OWN TEXT, NOT glm's: glm is not available
// where this is built, and nothing here is copied from it. The names, the memory layouts (tightly packed, matrices
// column-major) and the implicit conversions follow glm's documented interface. The ORDER of the floating-point
// operations is restated from what glm's generic (non-SIMD) templates do, the same statement as at the top of
// oracle/gsr_oracle.cpp:
//   mat4 * vec4   : (m[0]*v.x + m[1]*v.y) + (m[2]*v.z + m[3]*v.w)
//   mat3 * mat3   : R[c][r] = a[0][r]*b[c][0] + a[1][r]*b[c][1] + a[2][r]*b[c][2]
//   dot(vec4)     : (x*x + y*y) + (z*z + w*w);  normalize(v) = v * (1 / sqrt(dot(v, v)))
//   min(a, b)     : (b < a) ? b : a;  max(a, b) : (a < b) ? b : a
//   vector op vector, vector op scalar: component by component
// So what a build against these headers pins is the reference's own text; glm's operation orders stay a restatement.
// Names provided: vec2/3/4, ivec2, uvec2, mat3, mat4, int32, min, max, transpose, normalize (of a vec4), dot, inversesqrt.
#pragma once

#include <cmath>
#include <cstdint>
#include <type_traits>

namespace glm {

typedef std::int32_t int32;
typedef std::uint32_t uint32;

template <int L, typename T> struct vec;

template <typename T> struct vec<2, T> {
    union { T x, r; };
    union { T y, g; };
    vec() = default;
    constexpr vec(T s) : x(s), y(s) {}
    template <typename A, typename B> constexpr vec(A a, B b) : x(static_cast<T>(a)), y(static_cast<T>(b)) {}
    template <typename U> constexpr vec(const vec<2, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)) {}
    template <typename U> constexpr vec(const vec<3, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)) {}
    template <typename U> constexpr vec(const vec<4, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)) {}
    T& operator[](int i) { return i == 0 ? x : y; }
    const T& operator[](int i) const { return i == 0 ? x : y; }
};

template <typename T> struct vec<3, T> {
    union { T x, r; };
    union { T y, g; };
    union { T z, b; };
    vec() = default;
    constexpr vec(T s) : x(s), y(s), z(s) {}
    template <typename A, typename B, typename C>
    constexpr vec(A a, B b_, C c) : x(static_cast<T>(a)), y(static_cast<T>(b_)), z(static_cast<T>(c)) {}
    template <typename U> constexpr vec(const vec<3, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}
    template <typename U> constexpr vec(const vec<4, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)) {}
    T& operator[](int i) { return i == 0 ? x : (i == 1 ? y : z); }
    const T& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : z); }
};

template <typename T> struct vec<4, T> {
    union { T x, r; };
    union { T y, g; };
    union { T z, b; };
    union { T w, a; };
    vec() = default;
    constexpr vec(T s) : x(s), y(s), z(s), w(s) {}
    template <typename A, typename B, typename C, typename D>
    constexpr vec(A a_, B b_, C c, D d) : x(static_cast<T>(a_)), y(static_cast<T>(b_)), z(static_cast<T>(c)), w(static_cast<T>(d)) {}
    template <typename U, typename S>
    constexpr vec(const vec<3, U>& v, S s) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)), w(static_cast<T>(s)) {}
    template <typename U> constexpr vec(const vec<4, U>& v) : x(static_cast<T>(v.x)), y(static_cast<T>(v.y)), z(static_cast<T>(v.z)), w(static_cast<T>(v.w)) {}
    T& operator[](int i) { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
    const T& operator[](int i) const { return i == 0 ? x : (i == 1 ? y : (i == 2 ? z : w)); }
};

typedef vec<2, float> vec2;
typedef vec<3, float> vec3;
typedef vec<4, float> vec4;
typedef vec<2, int32> ivec2;
typedef vec<2, uint32> uvec2;

static_assert(sizeof(vec2) == 8 && sizeof(vec3) == 12 && sizeof(vec4) == 16 && sizeof(ivec2) == 8 && sizeof(uvec2) == 8,
              "tightly packed, as glm's defaults");
static_assert(std::is_trivially_default_constructible<vec4>::value && std::is_trivially_copyable<vec4>::value, "plain data");

// a scalar operand takes the vector's component type and does not take part in deduction
template <typename T> struct same { typedef T type; };

#define REF_GLM_VEC_OP(OP)                                                                                            \
    template <int L, typename T> inline vec<L, T> operator OP(const vec<L, T>& a, const vec<L, T>& b) {              \
        vec<L, T> r;                                                                                                  \
        for (int i = 0; i < L; ++i) r[i] = a[i] OP b[i];                                                              \
        return r;                                                                                                     \
    }                                                                                                                 \
    template <int L, typename T> inline vec<L, T> operator OP(const vec<L, T>& a, typename same<T>::type s) {        \
        vec<L, T> r;                                                                                                  \
        for (int i = 0; i < L; ++i) r[i] = a[i] OP s;                                                                 \
        return r;                                                                                                     \
    }                                                                                                                 \
    template <int L, typename T> inline vec<L, T> operator OP(typename same<T>::type s, const vec<L, T>& b) {        \
        vec<L, T> r;                                                                                                  \
        for (int i = 0; i < L; ++i) r[i] = s OP b[i];                                                                 \
        return r;                                                                                                     \
    }                                                                                                                 \
    template <int L, typename T> inline vec<L, T>& operator OP##=(vec<L, T>& a, const vec<L, T>& b) {                \
        for (int i = 0; i < L; ++i) a[i] = a[i] OP b[i];                                                              \
        return a;                                                                                                     \
    }
REF_GLM_VEC_OP(+)
REF_GLM_VEC_OP(-)
REF_GLM_VEC_OP(*)
#undef REF_GLM_VEC_OP

template <typename T, typename = typename std::enable_if<std::is_arithmetic<T>::value>::type>
constexpr T min(T a, T b) { return (b < a) ? b : a; }
template <typename T, typename = typename std::enable_if<std::is_arithmetic<T>::value>::type>
constexpr T max(T a, T b) { return (a < b) ? b : a; }
template <int L, typename T> inline vec<L, T> min(const vec<L, T>& a, const vec<L, T>& b) {
    vec<L, T> r;
    for (int i = 0; i < L; ++i) r[i] = (b[i] < a[i]) ? b[i] : a[i];
    return r;
}

template <typename T> inline T dot(const vec<4, T>& a, const vec<4, T>& b) { return (a.x * b.x + a.y * b.y) + (a.z * b.z + a.w * b.w); }
inline float inversesqrt(float x) { return 1.0f / std::sqrt(x); }
template <typename T> inline vec<4, T> normalize(const vec<4, T>& v) { return v * inversesqrt(dot(v, v)); }

template <int C, int R, typename T> struct mat;

template <typename T> struct mat<4, 4, T> {
    vec<4, T> value[4];     // columns
    mat() = default;
    vec<4, T>& operator[](int c) { return value[c]; }
    const vec<4, T>& operator[](int c) const { return value[c]; }
};

template <typename T> struct mat<3, 3, T> {
    vec<3, T> value[3];     // columns
    mat() = default;
    constexpr mat(T s) : value{vec<3, T>(s, 0, 0), vec<3, T>(0, s, 0), vec<3, T>(0, 0, s)} {}
    // nine scalars of any arithmetic types, column by column, each narrowed to T
    template <typename X0, typename Y0, typename Z0, typename X1, typename Y1, typename Z1, typename X2, typename Y2, typename Z2>
    constexpr mat(X0 x0, Y0 y0, Z0 z0, X1 x1, Y1 y1, Z1 z1, X2 x2, Y2 y2, Z2 z2)
        : value{vec<3, T>(x0, y0, z0), vec<3, T>(x1, y1, z1), vec<3, T>(x2, y2, z2)} {}
    // the upper-left 3 x 3 of a mat4
    constexpr mat(const mat<4, 4, T>& m) : value{vec<3, T>(m[0]), vec<3, T>(m[1]), vec<3, T>(m[2])} {}
    vec<3, T>& operator[](int c) { return value[c]; }
    const vec<3, T>& operator[](int c) const { return value[c]; }
};

typedef mat<3, 3, float> mat3;
typedef mat<4, 4, float> mat4;
static_assert(sizeof(mat3) == 36 && sizeof(mat4) == 64, "column-major, tightly packed");

template <typename T> inline vec<4, T> operator*(const mat<4, 4, T>& m, const vec<4, T>& v) {
    return (m[0] * v.x + m[1] * v.y) + (m[2] * v.z + m[3] * v.w);
}
template <typename T> inline mat<3, 3, T> operator*(const mat<3, 3, T>& a, const mat<3, 3, T>& b) {
    mat<3, 3, T> r;
    for (int c = 0; c < 3; ++c)
        for (int row = 0; row < 3; ++row) r[c][row] = a[0][row] * b[c][0] + a[1][row] * b[c][1] + a[2][row] * b[c][2];
    return r;
}
template <int N, typename T> inline mat<N, N, T> transpose(const mat<N, N, T>& m) {
    mat<N, N, T> r;
    for (int c = 0; c < N; ++c)
        for (int row = 0; row < N; ++row) r[c][row] = m[row][c];
    return r;
}

}  // namespace glm
