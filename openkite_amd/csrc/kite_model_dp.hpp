// kite_model_dp.hpp -- the kite ODE's derivative with respect to the 21
// identified aerodynamic coefficients (ident_kernels.hip), and the model
// constants of a kite_params row with those 21 replaced.
//
// In kite_rhs (kite_model.hpp) every one of the 21 enters exactly one of
//   LIFT (CL0, CLa, CLq), DRAG (CD0; CL0 and CLa through CLt^2 / (pi e AR)),
//   SF (CYb, CYdr, CYr, CYp), Zde (CLde), Lr (Clb, Cldr, Clr, Clp),
//   Mp (Cm0, Cma, Cmde, Cmq), Ny (Cnb, Cndr, Cnp, Cnr)
// linearly (quadratically through CLt^2), so a column of d f / d p is a scalar
// times a fixed direction of f[0:3] (the forces, through the wind-frame
// rotation) or of f[3:6] (the moments, through q(aoa) and J^-1).  Rows 6..12
// (kinematics) are zero.
//
// The airspeed, angle and pressure terms are written exactly as the value part
// of kite_rhs<Dual> computes them (fast_rcp included): inlined next to it, the
// compiler evaluates them once.
#pragma once
#include <stdint.h>

#include "kite_model.hpp"
#include "kite_nmpc/kite_nmpc.h"

namespace kite {

constexpr int NP = KITE_IDENT_NP;

// kite_params field (index into its 52 doubles) of identified parameter j
__host__ __device__ __forceinline__ int ident_field(int j) {
    // CL0 CLa_total CD0_total CYb Cm0 Cma Cnb Clb CLq Cmq CYr Cnr Clr CYp Clp Cnp CLde CYdr Cmde Cndr Cldr
    constexpr int8_t F[NP] = {15, 17, 21, 24, 26, 27, 29, 31, 32, 33, 34, 35, 36, 37, 38, 39, 40, 41, 42, 43, 44};
    return F[j];
}

// ModelConst of the row r52 (kite_params as 52 doubles) with the 21 identified
// fields taken from p21 instead (p21 == nullptr: the row's own).  The
// arithmetic of the host's make_model_const, unfused, so that host and device
// agree on every constant.
__host__ __device__ __forceinline__ ModelConst ident_model_const(const double* r52, const double* p21) {
#pragma clang fp contract(off)
    auto id = [&](int j) { return p21 ? p21[j] : r52[ident_field(j)]; };
    const double b = r52[0], c = r52[1], AR = r52[2], S = r52[3], mass = r52[10];
    const double Ixx = r52[11], Iyy = r52[12], Izz = r52[13], Ixz = r52[14], e_oswald = r52[20];
    const double rho = kRho;
    ModelConst m;
    m.inv_mass = 1.0 / mass;
    m.S = S; m.b = b; m.c = c;
    m.CL0 = id(0); m.CLa = id(1); m.CD0 = id(2);
    m.inv_pieAR = 1.0 / (3.14159265358979323846 * e_oswald * AR);
    m.kLq = 0.25 * id(8) * c * S * rho;
    m.CYb = id(3); m.CYdr = id(17); m.kSF = 0.25 * b * rho * S;
    m.CYr = id(10); m.CYp = id(13);
    m.CLde = id(16);
    m.Cl0 = r52[30]; m.Clb = id(7); m.Cldr = id(20); m.Clr = id(12); m.Clp = id(14);
    m.kRoll = 0.25 * rho * b * b * S;
    m.Cm0 = id(4); m.Cma = id(5); m.Cmde = id(18); m.Cmq = id(9);
    m.kPitch = 0.25 * S * c * c * rho;
    m.Cn0 = r52[28]; m.Cnb = id(6); m.Cndr = id(19); m.Cnp = id(15); m.Cnr = id(11);
    m.kYaw = 0.25 * S * b * b * rho;
    m.Ixx = Ixx; m.Iyy = Iyy; m.Izz = Izz; m.Ixz = Ixz;
    const double det = Ixx * Izz - Ixz * Ixz;
    m.Ji00 = Izz / det; m.Ji02 = -Ixz / det; m.Ji22 = Ixx / det; m.Ji11 = 1.0 / Iyy;
    m.Lt = r52[46]; m.Ks = r52[47]; m.Kd = r52[48]; m.rx = r52[49]; m.ry = r52[50]; m.rz = r52[51];
    m.half_rho = 0.5 * rho;
    return m;
}

// fp[0..5] = sc * d f[0..5] / d p_j at (x, u); d f[6..12] / d p_j = 0.
// WIND (kite_rhs<T, true>): the 21 enter only the aerodynamic forces and
// moments, which see the air-relative body velocity v_a = v - q^-1 (x) [0,W] (x) q,
// and v_a does not depend on them: the columns are the same scalars times the
// same directions with v_a in place of v (the rates w are the kite's own).  x
// then holds all 13 states (q = x[9..12]) and wnd the world-frame wind; v_a is
// written as the value part of kite_rhs<Dual, true> writes it.
template <bool WIND = false>
__device__ __forceinline__ void kite_rhs_dp(const ModelConst& P, const double* x, const double* u, int j, double sc,
                                            double* fp, const double* wnd = nullptr) {
    double vx = x[0], vy = x[1], vz = x[2];
    const double wx = x[3], wy = x[4], wz = x[5];
    if constexpr (WIND) {
        const double qw = x[9], qx = x[10], qy = x[11], qz = x[12];
        const double wwuu = qw * qw - (qx * qx + qy * qy + qz * qz);
        const double W0 = wnd[0], W1 = wnd[1], W2 = wnd[2];
        const double uv2 = 2.0 * (qx * W0 + qy * W1 + qz * W2);
        const double cx = qy * W2 - qz * W1, cy = qz * W0 - qx * W2, cz = qx * W1 - qy * W0;
        const double w2 = 2.0 * qw;
        vx = vx - (wwuu * W0 + uv2 * qx - w2 * cx);
        vy = vy - (wwuu * W1 + uv2 * qy - w2 * cy);
        vz = vz - (wwuu * W2 + uv2 * qz - w2 * cz);
    }
    const double dE = u[1], dR = u[2];
    // airspeed, angles, pressure: the value part of kite_rhs<Dual>
    const double V2 = vx * vx + vy * vy + vz * vz;
    const double V = sqrt(V2);
    const double sb = vy * fast_rcp(V + 1e-4);
    const double cb = sqrt(1.0 - sb * sb);
    const double ss = asin(sb);
    const double ax = vx + 1e-4;
    const double r2a = ax * ax + vz * vz;
    const double aoa = atan2(vz, ax);
    const double ira = fast_rcp(sqrt(r2a));
    const double ca = ax * ira, sa = vz * ira;
    const double qS = P.half_rho * V2 * P.S;
    const double CLt = P.CL0 + P.CLa * aoa;

    // d LIFT, d DRAG, d SF, d Zde, d Lr, d Mp, d Ny with respect to p_j
    double cL = 0.0, cD = 0.0, cS = 0.0, cZ = 0.0, cR = 0.0, cM = 0.0, cN = 0.0;
    const double qSb = qS * P.b, qSc = qS * P.c;
    const double dCD = 2.0 * CLt * P.inv_pieAR * qS;      // d DRAG / d CLt
    switch (j) {
        case 0: cL = qS; cD = dCD; break;                            // CL0
        case 1: cL = aoa * qS; cD = aoa * dCD; break;                // CLa
        case 2: cD = qS; break;                                      // CD0
        case 3: cS = ss * qS; break;                                 // CYb
        case 4: cM = qSc; break;                                     // Cm0
        case 5: cM = aoa * qSc; break;                               // Cma
        case 6: cN = ss * qSb; break;                                // Cnb
        case 7: cR = ss * qSb; break;                                // Clb
        case 8: cL = 0.25 * P.c * P.S * kRho * V * wy; break;        // CLq (kLq = 0.25 CLq c S rho)
        case 9: cM = P.kPitch * wy * V; break;                       // Cmq
        case 10: cS = wz * P.kSF * V; break;                         // CYr
        case 11: cN = wz * P.kYaw * V; break;                        // Cnr
        case 12: cR = wz * P.kRoll * V; break;                       // Clr
        case 13: cS = wx * P.kSF * V; break;                         // CYp
        case 14: cR = wx * P.kRoll * V; break;                       // Clp
        case 15: cN = wx * P.kYaw * V; break;                        // Cnp
        case 16: cZ = -(dE * qS); break;                             // CLde (Zde = -CLde dE qS)
        case 17: cS = dR * qS; break;                                // CYdr
        case 18: cM = dE * qSc; break;                               // Cmde
        case 19: cN = dR * qSb; break;                               // Cndr
        default: cR = dR * qSb; break;                               // Cldr
    }
    // forces: Fa = {cb a1x - sa Zde, sb a1x + SF, a1z + ca Zde},
    // a1x = -ca DRAG + sa LIFT, a1z = -sa DRAG - ca LIFT
    const double a1x = sa * cL - ca * cD;
    const double a1z = -(sa * cD) - ca * cL;
    const double k = sc * P.inv_mass;
    fp[0] = (cb * a1x - sa * cZ) * k;
    fp[1] = (sb * a1x + cS) * k;
    fp[2] = (a1z + ca * cZ) * k;
    // moments: m0 = ca Lr - sa Ny, m1 = Mp, m2 = sa Lr + ca Ny, then J^-1
    const double m0 = ca * cR - sa * cN;
    const double m2 = sa * cR + ca * cN;
    fp[3] = (P.Ji00 * m0 + P.Ji02 * m2) * sc;
    fp[4] = (P.Ji11 * cM) * sc;
    fp[5] = (P.Ji02 * m0 + P.Ji22 * m2) * sc;
}

}  // namespace kite
