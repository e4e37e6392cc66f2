// lx_geo.h -- a kernel geometry: G lanes per group x C columns per lane.  Every DP kernel is a template over that pair; between the
// planners and the launchers it travels as a Geo.  HIP-free.
#pragma once
#include <cstdint>
#include <type_traits>

namespace lx
{

struct Geo
{
    int16_t g = 0, c = 0; // lanes per group, columns per lane; {} = not chosen
    constexpr int  panel() const { return g * c; }             // columns of one panel
    constexpr int  groups() const { return g ? 64 / g : 0; }   // lane groups per wavefront
    constexpr bool chosen() const { return g != 0; }
    friend constexpr bool operator==(Geo a, Geo b) { return a.g == b.g && a.c == b.c; }
    friend constexpr bool operator!=(Geo a, Geo b) { return !(a == b); }
};
static_assert(sizeof(Geo) == 4 && std::is_trivially_copyable<Geo>::value, "a Geo takes the place of an int32 in the kernels' parameter blocks");

constexpr Geo kGeo16x10{16, 10}; // any query width (several panels), a profile per lane group
constexpr Geo kGeo8x19{8, 19};   // 152 columns
constexpr Geo kGeo16x13{16, 13}; // 208 columns

// The geometries a kernel family is instantiated for, and the one way from a run-time Geo to the compile-time pair: f(GeoT<G, C>{})
// for the entry of the list that equals `geo`, `miss` where there is none.
template <int G, int C>
struct GeoT
{
    static constexpr int g = G, c = C;
    static constexpr Geo geo() { return Geo{G, C}; }
};
template <class... Ts>
struct GeoList
{
    static constexpr int size = (int)sizeof...(Ts);
    static Geo at(int i) // (positions: lx_host_batch.cpp's bins)
    {
        Geo const all[] = {Ts::geo()...};
        return (i >= 0 && i < size) ? all[i] : Geo{};
    }
    static int index_of(Geo geo) // (-1: not in the list)
    {
        int i = 0, at = -1;
        (void)((geo == Ts::geo() ? (at = i, true) : (++i, false)) || ...);
        return at;
    }
};
template <class R, class F, class... Ts>
R geo_dispatch(GeoList<Ts...>, Geo geo, R miss, F && f)
{
    R r = miss;
    (void)((geo == Ts::geo() && ((r = f(Ts{})), true)) || ...);
    return r;
}

} // namespace lx
