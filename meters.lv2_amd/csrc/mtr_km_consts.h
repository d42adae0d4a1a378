// mtr_km_consts.h — the constants of Kmeterdsp as KMETER's reading series and SURROUND take them, computed once on the host
// (km_setup, mtr_kmeter_dsp.h).  Plain structs, no device code: the engine holds them as members (mtr_engine_impl.h).
#ifndef MTR_KM_CONSTS_H
#define MTR_KM_CONSTS_H

#include <stdint.h>

/* Kmeterdsp's constants, computed once on the host in double (kr = 1 - omega, ka = kr^4, kb = 1 - 4 omega, c = 4 omega ka) */
typedef struct mtr_km_consts {
	float   omega;                /* Kmeterdsp::init (kmeterdsp.cc:53) */
	int32_t hold;                 /* frames the peak is held (:52) */
	double  pw[3];                /* A = [[ka, 0], [c, kb]] per group of four frames */
	double  lkr, lkb;             /* log kr, log kb */
	double  kri, kai, kbi, kr3;   /* 1 / kr, 1 / ka, 1 / kb, kr^3 */
	double  ca, cb;               /* omega c / (ka - kb), omega (4 omega - c / (ka - kb)): the z2 weight of a frame is kr^(..) (ca ka^k + cb kb^k) */
	double  st1, sta, stb;        /* kr^-n, ka^-(n / 4), kb^-(n / 4): from one of a lane's steps to its next, n frames on */
} mtr_km_consts;

/* the constants of SURROUND (a lane step of km is a tile of k_sur_pieces): its K-meters', and what every lane of its correlations
 * would compute alike (r = 1 - w1, q = 1 - w2) */
typedef struct mtr_sur_consts {
	mtr_km_consts km;
	double lq, sq;                /* log q; q^-TILE: from tile to tile */
	double d1, d2, d4, d8, d64;   /* r^K to the powers of the wave scan */
} mtr_sur_consts;

#endif
