/*
 * rcmdyn.h -- C-ABI of the MI355X-native RegCM4 dynamical-core step engine.
 *
 * Drop-in boundary for the reference hot path:
 *
 *   reference seam                                  replaced by
 *   ---------------------------------------------   -------------------------------
 *   call tend        Main/mod_regcm_interface.F90:189 rcmdyn_tend()
 *   call bdyval      Main/mod_regcm_interface.F90:208 rcmdyn_bdyval()
 *   tend+bdyval loop Main/mod_regcm_interface.F90:172-228   rcmdyn_step()
 *   module state     Main/mod_atm_interface.F90:39-70 rcmdyn_put()/rcmdyn_get()
 *   bdyin (b0,bt)    Main/mod_bdycod.F90:654-889      put XxB_B0/BT + rcmdyn_set_time(xbctime)
 *   mkslice -> physics -> sums  Main/mod_tendency.F90:243,271,285-411
 *                    rcmdyn_tend_pre_physics() + get ATMS_* / put *PHY + rcmdyn_tend_post_physics()
 *   rcmtimer/dt/xbctime Main/mpplib/mod_runparams.F90 rcmdyn_set_time()/get_time()
 *   exchange*        Main/mpplib/mod_mppparam.F90:6065-13190  internal (local copies / RCCL)
 *   fatal('CFL VIOLATION') Main/mod_tendency.F90:702  return code + rcmdyn_last_error()
 *
 * Conventions
 *  - Every entry point returns 0 on success, non-zero on failure; the message of the
 *    last failure is available from rcmdyn_last_error().
 *  - Host arrays cross the boundary in the reference's Fortran layout: column-major
 *    (j fastest, then i, then k), with explicit GLOBAL index bounds j1:j2, i1:i2, k1:k2
 *    (Fortran 1-based, as allocated by getmem*: Share/mod_memutil.F90).  In C/numpy
 *    terms that is a C-order [k][i][j] array.  The engine copies the intersection of
 *    the host box with the tiles it owns; it never keeps a host pointer.
 *  - All arithmetic is fp64 (rkx = rk8, Share/mod_realkinds.F90:44-55).
 *  - No torch / HIP types appear in any signature.
 */
#ifndef RCMDYN_H
#define RCMDYN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RCMDYN_ABI_VERSION 6
#define RCMDYN_MAXKZ 64
#define RCMDYN_MAXSPLIT 4

/* Run/grid configuration.  Scalars mirror the namelist / mod_runparams globals that
 * the reference dyn core reads (Share/mod_dynparam.F90:453-476, Main/mod_params.F90:85-170,
 * Main/mpplib/mod_runparams.F90:97-232).  Vertical-mode constants are the outputs of the
 * host-side init (spinit/vmodes, Main/mod_split.F90:75-239, Main/mod_vmodes.F90:86-594). */
typedef struct rcmdyn_config {
  int32_t abi_version;          /* = RCMDYN_ABI_VERSION */
  /* global grid: jx (west-east dot points), iy (south-north), kz (levels) */
  int32_t jx, iy, kz;
  /* 2-D decomposition in tiles (set_nproc rule, Main/mpplib/mod_mppparam.F90:1133-1186);
   * tile t has cartesian location (t / nproc_i, t % nproc_i) = (j-coord, i-coord). */
  int32_t nproc_j, nproc_i;
  /* tiles owned by this engine instance: [tile_first, tile_first + tile_count) */
  int32_t tile_first, tile_count;
  /* dynamics options (defaults in brackets) */
  int32_t idynamic;             /* [1] hydrostatic, 2 = non-hydrostatic (MM5-type, sound) */
  int32_t iboudy;               /* [5] exponential relaxation (1 = linear) */
  int32_t idiffu;               /* [1] 1: 4th-order, 2: 9-point, 3: 6th-order flux-limited on each
                                   tile's last interior column (Main/mod_diffusion.F90:412-942) */
  int32_t ipgf;                 /* [0] */
  int32_t nsplit;               /* [2] */
  int32_t nspgx, nspgd;         /* [12,12] boundary relaxation band width */
  int32_t diffu_hgtf;           /* [1] topographic diffusion reduction */
  int32_t upstream_mode;        /* [1] */
  int32_t stability_enhance;    /* [1] */
  int32_t present_qc;           /* [0] ICBC carries qc (Main/mod_bdycod.F90:306-310) */
  /* scalars */
  double ds;                    /* grid spacing, km */
  double dtsec;                 /* namelist dt, s */
  double ptop;                  /* model top, cb */
  double gnu1, gnu2;            /* Robert-Asselin [0.0625] */
  double uoffc;                 /* [0.25] */
  double t_extrema;             /* [5] */
  double q_rel_extrema;         /* [0.2] */
  double ckh, adyndif;          /* [1,1] */
  double high_nudge, medium_nudge, low_nudge; /* [3,2,1] */
  double bdy_nm, bdy_dm;        /* [-1,-1] -> derived from dt */
  double dtbdys;                /* boundary interval, s [6*3600] */
  /* vertical structure */
  double sigma[RCMDYN_MAXKZ + 1];          /* full sigma levels, k = 1..kz+1 */
  /* split-explicit constants (after spinit scaling), Fortran index order noted */
  double zmatx[RCMDYN_MAXSPLIT][RCMDYN_MAXKZ];   /* zmatx(k,l) -> zmatx[l-1][k-1] */
  double zmatxr[RCMDYN_MAXSPLIT][RCMDYN_MAXKZ];  /* zmatxr(l,k) -> zmatxr[l-1][k-1] */
  double am[RCMDYN_MAXSPLIT][RCMDYN_MAXKZ];      /* am(k,l) -> am[l-1][k-1] */
  double tau[RCMDYN_MAXSPLIT][RCMDYN_MAXKZ];     /* tau(l,k) -> tau[l-1][k-1] */
  double varpa1[RCMDYN_MAXSPLIT][RCMDYN_MAXKZ + 1]; /* varpa1(l,k) -> varpa1[l-1][k-1] */
  double an[RCMDYN_MAXSPLIT];
  double hbar[RCMDYN_MAXSPLIT];
  double aam[RCMDYN_MAXSPLIT];
  double dtau[RCMDYN_MAXSPLIT];
  double sigmah[RCMDYN_MAXKZ + 1];
  double pd;                    /* vmodes reference p* (cb) */
  /* multi-process (RCCL) -- used only when tile_count < nproc_j*nproc_i */
  int32_t comm_rank, comm_size; /* process rank / size in the RCCL communicator */
  int32_t device;               /* HIP device ordinal, -1 = current */
  uint8_t comm_unique_id[128];  /* ncclUniqueId from rcmdyn_comm_unique_id() on rank 0 */
  /* non-hydrostatic core (idynamic = 2): nonhydroparam, Main/mod_params.F90:115-116,287-296 */
  int32_t ifupr;                /* [1] upper radiative boundary condition in sound */
  int32_t ifrayd;               /* [1] Rayleigh damping of the top levels */
  int32_t rayndamp;             /* [5] number of damped levels */
  int32_t nh_reserved;
  double nhbet, nhxkd;          /* [0.4, 0.1] Ikawa beta, divergence damping */
  double rayalpha0, rayhd;      /* [3e-4 1/s, 10000 m] */
  /* init_sound outputs (Main/mod_sound.F90:115-161), computed by the host once:
   * nh_dtsmax = dx / sqrt(gamma R max(t0)) / (1 + nhxkd), nh_xmsf = mean of msfx over the
   * interior cross points (the global sumall of :143-145) */
  double nh_dtsmax, nh_xmsf;
  /* cldparam relative-humidity clamps of the mkslice export (Main/mod_params.F90:331-332,
   * Main/mod_slice.F90:336-337) [rhmin 0.01, rhmax 1.01] */
  double rhmin, rhmax;
  /* physicsparam isladvec [0] (1 = semi-Lagrangian horizontal advection of the moisture,
   * Main/mod_sladvection.F90, both cores) and iqmsl [1] (its quasi-monotone limiter),
   * Main/mod_params.F90:100, 243-244 */
  int32_t isladvec, iqmsl;
  /* physicsparam ibltyp [1]: 2 = UW PBL, whose TKE the dyn step advects, diffuses, forecasts
   * and filters (Main/mod_tendency.F90:515-544, 1414-1425, 1545-1548) and bounds
   * (Main/mod_bdycod.F90:1166-1306, 2415-2530); uwparam nuk [5] (its diffusion factor,
   * Main/mod_params.F90:480); tkemin (uwtkemin = 1e-3, Main/pbllib/mod_pbl_uwtcm.F90:86,
   * Main/mod_pbl_interface.F90:68).  uwparam iuwvadv [0]: with ibltyp = 2, 1 selects the
   * PBL-aware vertical flux of the hydrometeors (vadv4d ind = 3, iqxvadv = 3,
   * Main/mod_tendency.F90:148-154, Main/mod_advection.F90:917-961), which reads the host's
   * KPBL field; ignored unless ibltyp = 2, as in the reference */
  int32_t ibltyp, iuwvadv;
  double nuk, tkemin;
  /* ABI 6.  physicsparam ipptls [1] and nqx, the number of moisture species param sets from
   * it (Main/mod_params.F90:1358-1366): nqx = 2 (qv, qc) for ipptls = 1 (SUBEX), nqx = 5 (qv,
   * qc, qi, qr, qs) for ipptls = 2 (WSM5 / Nogherotto-Tompkins).  Every hydrometeor
   * n = iqfrst..iqlst (qc and, with nqx = 5, qi, qr, qs) gets the qc chain of the dyn step:
   * hadvqx, vadv4d, diffu_x4d, the forecast and negative-value fix, filter_raw_4d with the zero
   * floor, bdyval's boundary copies and inflow/outflow lines; the total water load qcd (the sum
   * of the hydrometeors, Main/mod_tendency.F90:1107-1115) enters the geopotential's tvfac and
   * the NH water loading.  ipptls = 0 (no moisture scheme: the hydrometeor tendencies are never
   * summed, :331) and an nqx that does not match ipptls are refused. */
  int32_t ipptls, nqx;
  /* i_band = 1 (dimparam, hydrostatic core): the tropical band, periodic in j
   * (Main/mpplib/mod_mppparam.F90:1062, 1112-1114, 1131): no tile has a west or east boundary,
   * the tiles of the first and last tile column are neighbours (one tile in j is its own west
   * and east neighbour: its periodic exchange is a copy inside the tile), the cross grid takes
   * every j (:1351-1354: cross fields are defined on j = 1..jx), and only the south and north
   * rows relax to the boundary data (Main/mod_atm_interface.F90:435-457).  A put fills a band
   * tile's frame columns past either end of the period from the wrapped columns.  Refused for
   * idynamic = 2 and for values other than 0 and 1.
   * i_crm = 1 (cloud-resolving, periodic in j and i, Main/mpplib/mod_mppparam.F90:1063, 1132,
   * 1224-1257): the non-hydrostatic core over the band only.
   * ichem: this struct carries no tracer count, so a non-zero value is refused at rcmdyn_create;
   * the chemical tracers that tend advects, diffuses, relaxes, forecasts, fixes and filters
   * (Main/mod_tendency.F90:164, 198, 275, 548, 873) are declared after create with
   * rcmdyn_set_tracers (below), with ichem = 0 here. */
  int32_t i_band, i_crm, ichem;
} rcmdyn_config;

/* Field identifiers for put/get.  3-D fields have k = 1..kz unless noted. */
enum rcmdyn_field {
  /* prognostic state, coupled with p* exactly as the reference stores it */
  RCMDYN_ATM1_U = 0, RCMDYN_ATM1_V, RCMDYN_ATM1_T, RCMDYN_ATM1_QV, RCMDYN_ATM1_QC,
  RCMDYN_ATM2_U, RCMDYN_ATM2_V, RCMDYN_ATM2_T, RCMDYN_ATM2_QV, RCMDYN_ATM2_QC,
  RCMDYN_PSA, RCMDYN_PSB,                 /* 2-D (k1=k2=1) */
  RCMDYN_DSTOR, RCMDYN_HSTOR,             /* 2-D x nsplit (k = 1..nsplit) */
  /* static fields, as left by param (Main/mod_params.F90:1982-2002): map factors
   * already inverted, ht already converted to geopotential */
  RCMDYN_MSFX, RCMDYN_MSFD, RCMDYN_CORIOL, RCMDYN_HT,
  /* lateral boundary data (v3dbound / v2dbound b0, bt) */
  RCMDYN_XUB_B0, RCMDYN_XUB_BT, RCMDYN_XVB_B0, RCMDYN_XVB_BT,
  RCMDYN_XTB_B0, RCMDYN_XTB_BT, RCMDYN_XQB_B0, RCMDYN_XQB_BT,
  RCMDYN_XPSB_B0, RCMDYN_XPSB_BT,
  /* read-only diagnostics of the last tend */
  RCMDYN_PSC, RCMDYN_PTEN, RCMDYN_PSDOTA,
  RCMDYN_TTEN, RCMDYN_UTEN, RCMDYN_VTEN, RCMDYN_QVTEN, RCMDYN_QCTEN,
  RCMDYN_OMEGA, RCMDYN_QDOT /* k = 1..kz+1 */, RCMDYN_XKC, RCMDYN_PHI,
  /* non-hydrostatic state (coupled with p* like t): pressure perturbation (Pa), vertical
   * velocity on full levels (k = 1..kz+1), their boundary data */
  RCMDYN_ATM1_PP, RCMDYN_ATM2_PP, RCMDYN_ATM1_W, RCMDYN_ATM2_W,
  RCMDYN_XPPB_B0, RCMDYN_XPPB_BT, RCMDYN_XWWB_B0, RCMDYN_XWWB_BT,
  /* non-hydrostatic reference state and statics, as make_reference_atmosphere and
   * compute_full_coriolis_coefficients leave them (Main/mod_params.F90:2614-2741):
   * atm0 ps (2-D, p* in Pa), pr, t, rho, z (half levels), pf, rhof, zf (full levels, kz+1),
   * dpsdxm, dpsdym (2-D), dprddx, dprddy (dot, kz), ef, ddx, ddy, dmdx, dmdy (dot, 2-D),
   * ex, crx, cry (cross, 2-D) */
  RCMDYN_ATM0_PS, RCMDYN_ATM0_PR, RCMDYN_ATM0_T, RCMDYN_ATM0_RHO, RCMDYN_ATM0_Z,
  RCMDYN_ATM0_PF, RCMDYN_ATM0_RHOF, RCMDYN_ATM0_ZF,
  RCMDYN_DPSDXM, RCMDYN_DPSDYM, RCMDYN_DPRDDX, RCMDYN_DPRDDY,
  RCMDYN_EF, RCMDYN_DDX, RCMDYN_DDY, RCMDYN_DMDX, RCMDYN_DMDY, RCMDYN_EX, RCMDYN_CRX, RCMDYN_CRY,
  /* physics coupling (put): the pc_physic component of aten that the
   * host's physical_parametrizations produced (coupled with p*, like aten), added in tend's
   * sums exactly where the reference adds them (Main/mod_tendency.F90:285-314, 332-341,
   * 404-411).  Cross points for t, qv, qc, pp, w (w on kz+1 levels), dot points for u, v.
   * The engine holds no physics buffers until the first put of one of these; they then
   * persist (zero until put) and enter every later tend. */
  RCMDYN_TPHY, RCMDYN_QVPHY, RCMDYN_QCPHY, RCMDYN_UPHY, RCMDYN_VPHY, RCMDYN_PPPHY, RCMDYN_WPHY,
  /* atms slice fields (get, read-only) of mkslice, Main/mod_slice.F90:102-358, as the
   * physics reads them: filled by rcmdyn_tend_pre_physics from the state at the start of the
   * step; zero outside the index ranges the reference writes.  PF3D, WB3D, ZQ: kz+1 levels;
   * PS2D, RHOX2D: 2-D.  ZQ, ZA, DZQ only for idynamic = 1 (constant in the NH core). */
  RCMDYN_ATMS_UBX3D, RCMDYN_ATMS_VBX3D, RCMDYN_ATMS_UBD3D, RCMDYN_ATMS_VBD3D, RCMDYN_ATMS_TB3D,
  RCMDYN_ATMS_QVB3D, RCMDYN_ATMS_QCB3D, RCMDYN_ATMS_TV3D, RCMDYN_ATMS_PB3D, RCMDYN_ATMS_PF3D,
  RCMDYN_ATMS_PS2D, RCMDYN_ATMS_RHOX2D, RCMDYN_ATMS_TH3D, RCMDYN_ATMS_RHOB3D, RCMDYN_ATMS_TP3D,
  RCMDYN_ATMS_WPX3D, RCMDYN_ATMS_WB3D, RCMDYN_ATMS_ZQ, RCMDYN_ATMS_ZA, RCMDYN_ATMS_DZQ,
  RCMDYN_ATMS_QSB3D, RCMDYN_ATMS_RHB3D,
  /* device bdyin (put): the next ICBC record as read_icbc returns it
   * (Main/mod_bdycod.F90:469-480): u, v (m/s, dot), t (K), qv (kg/kg), ps (2-D, hPa; not read
   * for idynamic = 2), NH pp (Pa) and w (m/s, kz+1 levels), uncoupled; rcmdyn_bdyin converts
   * and couples it.  ATM0_PSDOT: atm0%psdot (2-D, Pa, dot points), the NH coupling factor of
   * u, v (:399). */
  RCMDYN_XUB_B1, RCMDYN_XVB_B1, RCMDYN_XTB_B1, RCMDYN_XQB_B1, RCMDYN_XPSB_B1, RCMDYN_XPPB_B1,
  RCMDYN_XWWB_B1, RCMDYN_ATM0_PSDOT,
  /* UW PBL turbulent kinetic energy (ibltyp = 2): atm1/atm2 tke, decoupled (m2/s2), kz+1
   * levels (Main/mod_atm_interface.F90), and the pc_physic tendency the UW scheme produces
   * (put, like the *PHY fields; added to the advective tendency, :530-531) */
  RCMDYN_ATM1_TKE, RCMDYN_ATM2_TKE, RCMDYN_TKEPHY,
  /* kpbl (put, ibltyp = 2): the PBL-top level index per cross point that the UW scheme sets
   * each step (Main/mod_atm_interface.F90:136, 1135: jci1:jci2 x ici1:ici2), as doubles
   * holding integers; read by the iuwvadv = 1 vertical flux.  A value above kz is refused
   * ('kpbl is greater than kz', Main/mod_advection.F90:923-925); below 4 the column keeps
   * the plain interpolated flux.  Zero until put. */
  RCMDYN_KPBL,
  /* ABI 6, nqx = 5 only (refused otherwise): the atm1/atm2 ice, rain and snow mixing ratios
   * qx(:,:,:,iqi|iqr|iqs), coupled with p* like qc; their pc_physic tendencies (put, like the
   * *PHY fields, :332-335); the mkslice export qxb3d(iqi|iqr|iqs) (get, like ATMS_QCB3D,
   * Main/mod_slice.F90:193-195) */
  RCMDYN_ATM1_QI, RCMDYN_ATM1_QR, RCMDYN_ATM1_QS, RCMDYN_ATM2_QI, RCMDYN_ATM2_QR, RCMDYN_ATM2_QS,
  RCMDYN_QIPHY, RCMDYN_QRPHY, RCMDYN_QSPHY,
  RCMDYN_ATMS_QXB3D_QI, RCMDYN_ATMS_QXB3D_QR, RCMDYN_ATMS_QXB3D_QS,
  RCMDYN_NFIELDS
};

typedef struct rcmdyn_engine rcmdyn_t;

/* Lifetime */
int rcmdyn_create(const rcmdyn_config* cfg, rcmdyn_t** out);
int rcmdyn_destroy(rcmdyn_t* h);
const char* rcmdyn_last_error(rcmdyn_t* h);    /* h may be NULL: last global error */

/* Decomposition (set_nproc, Main/mpplib/mod_mppparam.F90:1053-1371), host-only, no GPU:
 * fills cpus[2] = {cpus_j, cpus_i} for nproc ranks on a jx x iy grid. */
int rcmdyn_set_nproc(int32_t nproc, int32_t jx, int32_t iy, int32_t cpus[2]);
/* Tile extents in global indices: ext[8] = {jde1,jde2,ide1,ide2,jce1,jce2,ice1,ice2},
 * bdy[4] = {has_bdyleft, has_bdyright, has_bdybottom, has_bdytop}.  Host-only. */
int rcmdyn_tile_extent(int32_t jx, int32_t iy, int32_t nproc_j, int32_t nproc_i,
                       int32_t tile, int32_t ext[8], int32_t bdy[4]);
/* The same for the grid and decomposition of cfg (jx, iy, nproc_j, nproc_i), with the periodic
 * directions of i_band (j) and i_crm (i): a periodic direction has no boundary side and its
 * cross range takes every point (Main/mpplib/mod_mppparam.F90:1131-1132, 1340-1360), as the
 * engine's own tiles do.  rcmdyn_tile_extent is this call with i_band = i_crm = 0; a band or
 * CRM host picks its points with this one.  Returns non-zero for a tile or flag out of range,
 * and for i_crm = 1 without i_band = 1 (rcmdyn_create refuses that configuration).  Host-only. */
int rcmdyn_tile_extent_cfg(const rcmdyn_config* cfg, int32_t tile, int32_t ext[8], int32_t bdy[4]);

/* Communication plan of one rank, host-only (no GPU, no communicator): the halo messages and
 * collectives that rank cfg->comm_rank (one tile per rank: tile_first = comm_rank, tile_count
 * = 1, comm_size = nproc_j * nproc_i) issues for the first exchanges of the statics and the
 * boundary data, the initial bdyval after the state put (its slice exchange) and then nsteps x
 * (tend + bdyval), in issue order.  Record q is
 * ops[7q .. 7q+6] = {call, kind, channel, dir, peer, count, signature}: call = the rank's
 * communication call number; kind 1 = one grouped send/receive (one record per message), 2 =
 * all-reduce sum (f64), 3 = all-reduce max (i32), 4 = all-reduce max (f64); channel 0/1 = the
 * engine stream that issues it (over RCCL both share the job's communicator, the second
 * ordered after the first); dir 0 send, 1 receive, -1 collective; peer = rank
 * (-1 for collectives); count = doubles (collectives: elements); signature = hash of the
 * message's box shapes (0 for collectives).  *count = records in the plan (at most cap are
 * written).  Every message A sends B must be the receive B posts from A, in the same order on
 * the same channel, which a multi-rank job needs and tests check.  The plan models no put
 * between steps: a KPBL put (ibltyp = 2, iuwvadv = 1, hydrostatic) adds one width-1 exchange
 * of kpbl before the next tend, on every rank alike. */
int rcmdyn_exchange_plan(const rcmdyn_config* cfg, int32_t nsteps, int64_t* ops, int64_t cap, int64_t* count);
/* Halo/compute overlap of the hydrostatic step, host-only (no GPU): for each of the first cap
 * tiles this engine would own, out[6q .. 6q+5] = {k_columns points in the part-1 rectangle R,
 * k_columns points, k_momentum points of its part-1 blocks, k_momentum points, k_scalars points
 * of its part-1 blocks, k_scalars points}: the share of each kernel that runs beside the
 * prologue exchange (0 when the step does not overlap: one tile, NH, idiffu = 3). */
int rcmdyn_overlap_shares(const rcmdyn_config* cfg, int32_t* out, int32_t cap);

/* State transfer (host <-> device), Fortran layout, global index bounds. */
int rcmdyn_put(rcmdyn_t* h, int32_t field, const double* src,
               int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
int rcmdyn_get(rcmdyn_t* h, int32_t field, double* dst,
               int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
/* Step failures (CFL VIOLATION, SLADVECTION) are detected on the device.  rcmdyn_step and
 * rcmdyn_tend report a failed step at most 2 steps late (one-rank jobs) or one reduction
 * interval (8 steps) late (RCCL jobs), so they never wait for the stream per step;
 * rcmdyn_get and rcmdyn_diagnostics wait for the stream and report any failure of the steps
 * issued so far before copying anything (with RCCL: the job-wide words already reduced and
 * this rank's own flags; no collective is issued, so a rank may call them alone). */

/* rcm_timer state: lcount (steps done), dt (current leapfrog dt, s), xbctime (s since
 * the current boundary interval started). */
int rcmdyn_set_time(rcmdyn_t* h, int64_t lcount, double dt, double xbctime);
int rcmdyn_get_time(rcmdyn_t* h, int64_t* lcount, double* dt, double* xbctime);

/* The hot path. */
int rcmdyn_tend(rcmdyn_t* h);                  /* one mod_tendency::tend */
/* tend split at the reference's call of physical_parametrizations (Main/mod_tendency.F90:
 * 271): pre_physics runs surface_pressures, decouple, compute_omega, mkslice (device export
 * of the ATMS_* fields) and new_pressure; the host then runs its physics on the ATMS_*
 * fields, puts the *PHY tendencies, and post_physics runs the rest of tend.  pre + post is
 * bit-identical to rcmdyn_tend with the same *PHY contents. */
int rcmdyn_tend_pre_physics(rcmdyn_t* h);
int rcmdyn_tend_post_physics(rcmdyn_t* h);
int rcmdyn_bdyval(rcmdyn_t* h);                /* one mod_bdycod::bdyval */
/* mod_bdycod::bdyin from read_icbc on (Main/mod_bdycod.F90:654-889), on the device:
 * b0 <- b1; the record put into the XxB_B1 fields becomes the new b1 (p* = ps/10 - ptop,
 * exchange, psc2psd, couple u, v with p* on dot points and t, qv (pp, w) with p*, exchange);
 * bt = (b1 - b0)/dtbdys on the ga ranges (timeint); xbctime = 0.  The reference's init_bdy
 * (:280-650) reads b0 and b1: call rcmdyn_bdyin twice, with the record at the start and the
 * one dtbdys later. */
int rcmdyn_bdyin(rcmdyn_t* h);
int rcmdyn_step(rcmdyn_t* h, int32_t nsteps);  /* nsteps x (tend + bdyval), graph-replayed */
/* Waits for the device and reports a failure of any step issued so far.  In RCCL mode it is
 * COLLECTIVE (it max-reduces the step error flags over the job so that every rank stops at
 * the same call): every rank must call it, as every rank calls rcmdyn_step and
 * rcmdyn_reductions.  In RCCL mode a step failure (CFL / NaN / departure point) this rank's
 * own flags hold is sticky at the host read points (get, diagnostics): it is reported there
 * before the job-wide reduction carries it, and again at every later read, until
 * rcmdyn_set_time (the host's restart from a SAV state) clears the flags.  The reference's
 * fatal ends the job there (Main/abort.F90:20-36), as a host should. */
int rcmdyn_synchronize(rcmdyn_t* h);

/* Diagnostics of the last tend: out[0]=ptntot, out[1]=pt2tot (Bleck noise sums of the
 * owned tiles, Main/mod_tendency.F90:1449-1459), out[2]=1 if ptntot is NaN. */
int rcmdyn_diagnostics(rcmdyn_t* h, double out[4]);

/* The 3-hourly report of tend and sound (syncro_rep, Main/mod_tendency.F90:705-725,
 * Main/mod_sound.F90:634-646), reduced over every tile of the job (sumall / maxall: the
 * engine's own tiles, then RCCL across ranks; collective in RCCL mode -- every rank calls
 * it): out[0] = sum of |pten| (ptntot), out[1] = sum of the 2nd time derivative of p*
 * (pt2tot) over the interior points of the last step (the host multiplies both by its
 * rptn = 1/npoints, :715-716); out[2] = NH: the maximum sigma-velocity CFL of the last
 * acoustic sub-step (maxall(cfl), :637), 0 for the hydrostatic core. */
int rcmdyn_reductions(rcmdyn_t* h, double out[3]);

/* Which runtime libraries the engine's calls are bound to: "hip=<path>; rccl=<path>
 * (<version>)" into buf (NUL-terminated, at most len bytes).  In a PyTorch process the
 * already-loaded libamdhip64.so.7 / librccl.so.1 (torch's copies, same sonames) are the
 * ones bound when torch was imported first; otherwise ROCm's (/opt/rocm/lib). */
int rcmdyn_runtime_info(char* buf, int32_t len);

/* Multi-process: rank 0 creates the id, the host broadcasts it (MPI / torch.distributed),
 * every rank passes it in rcmdyn_config.comm_unique_id. */
int rcmdyn_comm_unique_id(uint8_t out[128]);

/* Wall-clock of device work: average ms per step of the last rcmdyn_step call measured
 * with HIP events on the engine's compute stream. */
int rcmdyn_last_step_ms(rcmdyn_t* h, double* ms);

/* Tendency diagnostics (TTEN..QCTEN, OMEGA, XKC of rcmdyn_field): off by default.  When on,
 * every tend also stores the per-point tendencies the reference accumulates in aten
 * (Main/mod_tendency.F90:259-400) for rcmdyn_get; when off those gets fail.  The prognostic
 * results are identical either way. */
int rcmdyn_set_diagnostics(rcmdyn_t* h, int32_t on);

/* Tendency budget of t and qv (the reference's idiag = 1): off by default.  When on, every tend
 * also adds, for each phase of tend, the change of the running dynamic tendency over that phase
 * times rw to an accumulator, as mod_tendency does around its phases with ten0 / qen0 and
 * ten2diag (Main/mod_tendency.F90:1276-1279, 1332-1376, 1465-1487, 1521-1530, 1557-1560,
 * 1603-1606, 1673-1676, 2123-2175): tdiag / qdiag %adh (horizontal advection), adv (vertical
 * advection), adi (adiabatic), bdy (boundary relaxation), dif (horizontal diffusion), the
 * tten_* / qten_* variables of the ATM file (Main/mod_output.F90:668-871).  The accumulators
 * are coupled with p* like aten, live on the interior cross points jci1:jci2 x ici1:ici2,
 * k = 1..kz, and are zero elsewhere.  Each term is the rounded difference of two running sums,
 * not the separately evaluated term.  With the reference's quirks: the NH core (ithadv = 1)
 * books its whole theta path under T_ADH, never touches T_ADV and leaves T_ADI exactly 0;
 * hydrostatic Q_ADI is exactly 0, NH Q_ADI is atmx%qx * cr; with isladvec = 1 Q_ADH is the
 * semi-Lagrangian start; iboudy = 4 books the sponge value itself under *_BDY (no ten0), iboudy
 * 1 and 5 the nudging increment, iboudy 0, 2, 3 nothing.  The *PHY tendencies, the NH Rayleigh
 * damping and the physics terms (tbl, con, lsc, rad) stay the host's and enter no term.  The
 * prognostic results and the TTEN.. diagnostics are identical with the budget on or off. */
enum rcmdyn_budget_term {
  RCMDYN_BUD_T_ADH = 0, RCMDYN_BUD_T_ADV, RCMDYN_BUD_T_ADI, RCMDYN_BUD_T_BDY, RCMDYN_BUD_T_DIF,
  RCMDYN_BUD_Q_ADH, RCMDYN_BUD_Q_ADV, RCMDYN_BUD_Q_ADI, RCMDYN_BUD_Q_BDY, RCMDYN_BUD_Q_DIF,
  RCMDYN_NBUDGET
};
/* Switches the budget on or off.  rw is the host's alarm_out_atm%rw (model_timestep / atmfrq,
 * Main/mpplib/mod_timer.F90:300), applied from the next tend on; idgq is the species of qdiag
 * and must be iqv = 1, the reference's default (another species is refused: the reference
 * itself mixes iqv into that path, Main/mod_tendency.F90:1384-1391, 1559).  A non-finite or
 * non-positive rw is refused.  The ten accumulators are allocated, zeroed, on the first call
 * with on != 0 and keep their contents across later calls (off and on again, a new rw).  Waits
 * for the device like rcmdyn_set_diagnostics. */
int rcmdyn_set_budget(rcmdyn_t* h, int32_t on, int32_t idgq, double rw);
/* Copies one accumulator (term: enum rcmdyn_budget_term) to the host, layout and global bounds
 * as in rcmdyn_get; like rcmdyn_get it waits for the stream and reports step failures first.
 * Fails while the budget is off and for a term out of range.  There is no put: the reference
 * does not carry these sums through its SAV files either, so a restarted run starts them at
 * zero. */
int rcmdyn_get_budget(rcmdyn_t* h, int32_t term, double* dst,
                      int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
/* Zeroes the ten accumulators (mod_output's tdiag%x = d_zero after it wrote them). */
int rcmdyn_reset_budget(rcmdyn_t* h);

/* Mass check of tend (the reference's `if ( debug_level > 0 ) call massck`,
 * Main/mod_tendency.F90:415, Main/mod_massck.F90:190-306, the idynamic /= 3 branch): off by
 * default.  When on, every tend also sums, over the tiles this engine owns, from atm1 and sfs%psa
 * as they stand after tend's prologue exchange:
 *   drymass = (sum_k (sum_{jci,ici} psa) * dsigma(k)) * dxsq * 1000 * regrav
 *   qmass   = (sum_{n=1..nqx} sum_k (sum_{jci,ici} atm1%qx(:,:,k,n)) * dsigma(k)) * dxsq * 1000 * regrav
 *   dryadv  = the dry-air flux through the boundary lines a tile has, +- dt*3.e4*dsigma(k)*dx*regrav*f,
 *             west/east f = atm1%u(jde1|jde2,i+1,k) + atm1%u(jde1|jde2,i,k), i = ice1..ice2,
 *             south/north f = atm1%v(j+1,ide1|ide2,k) + atm1%v(j,ide1|ide2,k), j = jci1..jci2;
 *             inflow positive; dt is the clock's leapfrog dt before the tend (rcmdyn_get_time)
 *   qadv    = the same with f * atm1%qx / psa of the adjacent cross point, over every species
 * A periodic side (i_band, i_crm) has no line.  One record of six doubles per tend,
 *   { lcount, dt, drymass, dryadv, qmass, qadv }     (lcount, dt: the clock before the tend)
 * goes to a ring of cap records on the device, inside the captured step: nothing is copied and
 * no collective is issued until rcmdyn_get_massck.  The sums are fixed trees (no atomics): the
 * same run gives the same bits.  The prognostic results are identical with the check on or off,
 * and with it off the step issues no launch of it.  The scalar part of massck (the drift in %,
 * the 24-hour means, the daily report; :69-70, 312-364) stays the host's, with its rain and
 * evaporation sums (regcm_amd/massck.py restates it).
 *
 * rcmdyn_set_massck: on != 0 switches the check on with an empty log of cap records, 1 <= cap <=
 * 65536 (refused otherwise, the switch staying as it was; cap is not read when on == 0).  A call
 * that repeats the current on and cap keeps the log.  Waits for the device like
 * rcmdyn_set_budget.
 * rcmdyn_get_massck: like rcmdyn_get it waits for the stream and reports step failures first;
 * then copies the records of the tends since the previous rcmdyn_get_massck (or the switch-on)
 * to out[6 * cap], oldest first, at most min(cap, the log's cap) of them, the newest ones;
 * *count is the number copied, *lost the number of older ones the ring overwrote or out had no
 * room for.  The log is empty afterwards.  Fails with "the mass check is off" while it is off.
 * On a job whose tiles span ranks every rank's log holds its own tiles' sums, and this call adds
 * the four sums of each record over the job (the reference's sumall): it is then collective
 * like rcmdyn_reductions, every rank calling it with the same cap after the same tends. */
int rcmdyn_set_massck(rcmdyn_t* h, int32_t on, int32_t cap);
int rcmdyn_get_massck(rcmdyn_t* h, double* out, int32_t cap, int32_t* count, int64_t* lost);

/* SUBEX large-scale condensation inside tend (the reference's `call condtq` for ipptls = 1,
 * Main/mod_tendency.F90:336-349, Main/mod_micro_interface.F90:382-493, the idynamic /= 3 branch):
 * off by default.  When on, every tend applies, after it summed the tendencies of t, qv, qc (and
 * NH pp) and before the NH Rayleigh damping and the forecasts, the one-step condensation /
 * evaporation adjustment with partial cloud cover at every interior cross point.  It reads the
 * step's own totals, sfs%psc, atms%qsb3d of the step's start (formed at the point as mkslice
 * does) and the host's rh0adj, and adds the coupled increments -psc*tmp2 (qv), +psc*tmp2 (qc),
 * +psc*tmp2*wlh*rcpd (t) where |tmp2| > dlowval.  TTEN / QVTEN / QCTEN then include the term, as
 * aten(pc_total) does after :345-349.  The operations and their order are the Fortran text's.
 *
 * rcmdyn_set_condtq: conf is subexparam's condensation efficiency (Main/mod_params.F90:326,
 * default 1.0).  Refused for ipptls != 1 and for conf outside (0, 1], the switch staying as it
 * was.  Waits for the device like rcmdyn_set_budget.
 * rcmdyn_put_rh0adj: the adjusted relative-humidity threshold the host's cldfrac produces inside
 * physical_parametrizations (Main/mod_micro_interface.F90:353-356), cross points, kz levels,
 * layout and bounds as in rcmdyn_put.  A value outside [0, 0.99999] (the reference's clamp; 1 -
 * rh0adj is a divisor) refuses the whole put.  The buffer persists like the *PHY ones; on the
 * split path the host puts it between rcmdyn_tend_pre_physics and rcmdyn_tend_post_physics.  A
 * decomposed job's host passes the values of the tile's ghost ring too, as for the *PHY fields;
 * the frame columns of a band (rows in CRM mode) past either end of the period are filled from
 * the wrapped index, as rcmdyn_put does.
 * A tend with condtq on fails until, since the switch-on, one put has covered every level of
 * every interior cross point of the engine's tiles and of their ghost rings (for one tile: jci1
 * .. jci2, ici1 .. ici2, 1 .. kz); puts of smaller boxes update the buffer before and after it.
 * rcmdyn_get_condtq: the held rh0adj, or the last tend's increments of t, qv, qc (coupled, as
 * aten(.., pc_physic) holds them after condtq; the host feeds tdiag%lsc / qdiag%lsc from them,
 * :351-354); the increments are written to dst on the interior cross points only.  Fails while
 * the switch is off. */
enum rcmdyn_condtq_term {
  RCMDYN_CONDTQ_RH0ADJ = 0, RCMDYN_CONDTQ_T, RCMDYN_CONDTQ_QV, RCMDYN_CONDTQ_QC, RCMDYN_NCONDTQ
};
int rcmdyn_set_condtq(rcmdyn_t* h, int32_t on, double conf);
int rcmdyn_put_rh0adj(rcmdyn_t* h, const double* src,
                      int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
int rcmdyn_get_condtq(rcmdyn_t* h, int32_t term, double* dst,
                      int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);

/* SUBEX on the device (ipptls = 1): cldfrac with subex_cldfrac (Main/mod_micro_interface.F90:
 * 211-362, Main/cloudlib/mod_cloud_subex.F90:46-107) and the rain columns of subex (Main/microlib/
 * mod_micro_subex.F90:99-393), off by default.  When on, the engine forms the large-scale cloud
 * fraction fcc, the cloud fraction and in-cloud liquid water merged with cucloud's, rh0adj, and the
 * autoconversion / accretion / evaporation of rain from the top level down, from the mkslice
 * export of the same tend (tb3d, pb3d, pf3d, qxb3d qv / qc, rhob3d, rhb3d) and p*b.  The rain
 * columns' coupled increments of t, qv, qc (LSC_T, LSC_QV, LSC_QC: the text's update of a zero
 * tendency, the idynamic 1 / 2 form with * psb) enter the tend as pc_physic tendencies: a
 * pointwise pass forms TPHY + LSC_T, QVPHY + LSC_QV, QCPHY + LSC_QC and the tendency kernels read
 * those sums (the increments themselves where no *PHY was put).  The reference accumulates in
 * place in the order its schemes run; the sum here rounds once more where the host's TPHY carries
 * schemes from both before and after the microphysics, and has the same bits otherwise.
 * With condtq on as well, condtq reads the device's rh0adj of the same tend: no rcmdyn_put_rh0adj
 * is needed (it is refused, the host's values would be overwritten), and rcmdyn_get_condtq(RH0ADJ)
 * returns the device's field.  rh0adj and the increments travel one point wide to the tiles' rings:
 * the first tend on 2 x 2 tiles gives the bits of one tile, later steps those of the same tiles fed
 * by the host route (tiles and one tile part at the reference's tile-dependent negative-moisture
 * sweep, with or without subex).
 *
 * Whole mode: rcmdyn_tend / rcmdyn_step run the mkslice export and the subex kernels where the
 * reference calls physical_parametrizations (after mkslice, before the tendencies), inside the
 * replayed graphs.  Split mode: rcmdyn_tend_pre_physics, then rcmdyn_physics_subex, then
 * rcmdyn_tend_post_physics, so the host can fetch CLDFRA / CLDLWC for its radiation in between; if
 * the host did not call rcmdyn_physics_subex, rcmdyn_tend_post_physics runs it first.  It runs
 * once per tend: a second call before the post phase does nothing.
 *
 * rcmdyn_set_subex: rhmax, rhmin (the run's clamps, rhmin < rhmax), tc0 (K), larcticcorr (0 / 1),
 * iconvlwp (0 / 1) and rem (1: also remrat and rembc for the chemistry, the reference's ichem =
 * 1).  icldfrac, icldmstrat and lsecind are the host's settings of options that are not built:
 * icldfrac other than 0, icldmstrat = 1 (needs th700 and iveg) and lsecind = 1 (the aerosol second
 * indirect effect, needs ccn) are refused by name, as is ipptls other than 1; the switch then
 * stays as it was.  Buffers are allocated at the switch-on and freed at the switch-off; the
 * accumulators and tables of an earlier switch-on are gone.  Waits for the device like
 * rcmdyn_set_budget; the order of this call, rcmdyn_set_condtq and rcmdyn_set_tracers is free.
 *
 * Fields (enum rcmdyn_subex_field), cross points, layout and bounds as in rcmdyn_put / rcmdyn_get:
 *   RH0, QCK1, CGUL, CEVAP, CACCR   put, 2-D: the tables of Main/mod_params.F90:2455-2480.  A run
 *                         with subex on fails, naming the first one missing, until a put of each
 *                         has covered every interior cross point; values must be finite
 *   CU_CLDFRA, CU_CLDLWC  put, kz levels: cucloud's cloud fraction (finite, in [0, 1]) and liquid
 *                         water, zero until put
 *   RAINNC, LSMRNC        put and get, 2-D: the accumulated large-scale rain (kg/m2) and its rate
 *                         sum; the host zeroes them by a put, as the reference does at output
 *   FCC, CLDFRA, CLDLWC, RH0ADJ, LSC_T, LSC_QV, LSC_QC (kz levels), TRRATE (2-D)   get only
 *   REMRAT, REMBC         get only, kz levels, with rem on
 * Gets write the interior cross points of dst only. */
enum rcmdyn_subex_field {
  RCMDYN_SUBEX_RH0 = 0, RCMDYN_SUBEX_QCK1, RCMDYN_SUBEX_CGUL, RCMDYN_SUBEX_CEVAP, RCMDYN_SUBEX_CACCR,
  RCMDYN_SUBEX_CU_CLDFRA, RCMDYN_SUBEX_CU_CLDLWC, RCMDYN_SUBEX_RAINNC, RCMDYN_SUBEX_LSMRNC,
  RCMDYN_SUBEX_FCC, RCMDYN_SUBEX_CLDFRA, RCMDYN_SUBEX_CLDLWC, RCMDYN_SUBEX_RH0ADJ,
  RCMDYN_SUBEX_LSC_T, RCMDYN_SUBEX_LSC_QV, RCMDYN_SUBEX_LSC_QC, RCMDYN_SUBEX_TRRATE,
  RCMDYN_SUBEX_REMRAT, RCMDYN_SUBEX_REMBC, RCMDYN_NSUBEX
};
int rcmdyn_set_subex(rcmdyn_t* h, int32_t on, double rhmax, double rhmin, double tc0, int32_t larcticcorr,
                     int32_t iconvlwp, int32_t rem, int32_t icldfrac, int32_t icldmstrat, int32_t lsecind);
int rcmdyn_put_subex(rcmdyn_t* h, int32_t field, const double* src,
                     int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
int rcmdyn_get_subex(rcmdyn_t* h, int32_t field, double* dst,
                     int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
int rcmdyn_physics_subex(rcmdyn_t* h);

/* Chemical and aerosol tracers (the reference's ichem = 1): the chi chain of tend and bdyval on
 * the device.  tend decouples (atmx%chi = atm1%chi * rpsa, no floor), advects (hadvtr; vadv4d
 * with itrvadv = 2, threshold mintr * ps, or 3 under ibltyp = 2 with iuwvadv = 1), relaxes
 * (nudge_chiten, iboudy 1 or 5), diffuses (diffu_x on chib3d), sums with chiphy, forecasts,
 * fixes negative values (0.1 * the mean of the nine |chi|, serially in the reference's order)
 * and filters (RAW, gnu2, 0.53, zero floor) every tracer on the step's own mass fluxes, qdot and
 * xkc (Main/mod_tendency.F90:548-586, 1027-1032, 1393-1412, 1502-1512, 1539-1543); bdyval runs
 * chem_bdyval_coupled (Main/chemlib/mod_che_bdyco.F90:565-758).  Tracers are passive: no other
 * field of the step reads them.  The chemistry itself (sources, deposition, the gas-phase
 * mechanism, cumulus transport) stays the host's and enters as the pc_physic tendency TR_PHY.
 *
 * Fields of one tracer, coupled with p* like qc, kz levels, cross points:
 *   TR_ATM1, TR_ATM2   chia, chib (put and get; part of the SAV state)
 *   TR_PHY             chiphy (put only; persistent, zero until put)
 *   TR_B0, TR_BT       chib0, chibt as che_init_bdy / chem_bdyin leave them (put and get); the
 *                      host puts them at each boundary interval
 *   TR_CHIB3D          mkslice's chib3d = max(chib / psb, 0) (get only; filled by
 *                      rcmdyn_tend_pre_physics, Main/mod_slice.F90:196-200) */
enum rcmdyn_tracer_field {
  RCMDYN_TR_ATM1 = 0, RCMDYN_TR_ATM2, RCMDYN_TR_PHY, RCMDYN_TR_B0, RCMDYN_TR_BT, RCMDYN_TR_CHIB3D,
  RCMDYN_NTRFIELDS
};
/* The most tracers one engine carries: above the reference's largest chemsimtype preset (52,
 * Main/chemlib/mod_che_common.F90:269-397).  The bound only sizes host tables. */
#define RCMDYN_MAXTR 96
/* Declares ntr tracers (ntr = 0: switches the family off and frees its buffers; the state of
 * the tracers is lost).  Goes through the engine's state machine like rcmdyn_set_condtq: pending
 * work is flushed, the device is waited for and the captured graphs are dropped.  A call that
 * repeats the current ntr keeps the buffers.  Refused, the family staying as it was, for
 *   ntr < 0 or ntr > RCMDYN_MAXTR;
 *   ichebdy != 1: the ichebdy = 0 relaxation indexes tile-local rows (Main/chemlib/
 *     mod_che_bdyco.F90:808-896), so its result depends on the decomposition; not built;
 *   idiffu = 3: the tracers have no sixth-order column planes;
 *   isladvec = 1: slhadv_x of chi is not built. */
int rcmdyn_set_tracers(rcmdyn_t* h, int32_t ntr, int32_t ichebdy);
/* One field (enum rcmdyn_tracer_field) of tracer itr = 1..ntr; layout, bounds and box rules as in
 * rcmdyn_put / rcmdyn_get, a band's wrapped frame columns included.  Refused before
 * rcmdyn_set_tracers (or after ntr = 0), for itr out of range, for a put of TR_CHIB3D, a get of
 * TR_PHY, and a get of TR_CHIB3D before the first rcmdyn_tend_pre_physics. */
int rcmdyn_put_tracer(rcmdyn_t* h, int32_t field, int32_t itr, const double* src,
                      int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
int rcmdyn_get_tracer(rcmdyn_t* h, int32_t field, int32_t itr, double* dst,
                      int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
/* nudge_chiten's tables cefc(ib, k) and cegc(ib, k), ib = 1..nspgx, k = 1..kz, Fortran order (ib
 * fastest).  The reference allocates them (Main/chemlib/mod_che_bdyco.F90:110-111) and assigns
 * them nowhere, so its tracer relaxation adds zero: both start at zero here and stay so until
 * put.  Read only for iboudy 1 and 5 (Main/mod_tendency.F90:1506). */
int rcmdyn_put_tracer_nudge(rcmdyn_t* h, const double* cefc, const double* cegc);

/* Cumulus mixing of the tracers inside tend (the reference's `call cumtran(atm1%chi,atm2%chi)` for
 * ichcumtra = 1, Main/mod_tendency.F90:595-603, Main/chemlib/mod_che_cumtran.F90:118-167): off by
 * default.  When on, a tend whose clock before its advance has lcount > 0 (rcmtimer%integrating)
 * and lcount % ncum == 0 (syncro_cum%act, ncum = dtcum / dtsec in steps) mixes every tracer, after
 * the time filter and before the clock advance, at the interior cross points where DOTRAN is set
 * and KTOP > 0: with kctop = max(KTOP, 4), deltas and the two column means are summed over
 * k = kctop .. kz in that order, and both time levels take x * (1 - cumfrc) + cumfrc * xbar /
 * deltas there.  kctop > kz leaves the column as it is.  The operations and their order are the
 * Fortran text's.  The producers of the three inputs (init_cumtran's mask from cveg2d and icup, the
 * convection scheme's kcumtop and convcldfra) stay the host's.
 *
 * rcmdyn_set_cumtran: refused while no tracers are declared and for ncum < 1, the switch staying
 * as it was.  Goes through the engine's state machine like rcmdyn_set_condtq (ncum is a kernel
 * argument: the captured graphs are dropped).  A switch-on from off starts from zeroed inputs
 * (KTOP = 0 mixes nothing, so no tend waits for a put).  rcmdyn_set_tracers with another count
 * switches it off and frees its buffers.
 * rcmdyn_put_cumtran / rcmdyn_get_cumtran: one input (enum rcmdyn_cumtran_field), layout, bounds
 * and box rules as rcmdyn_put_tracer (the 2-D fields with k1 = k2 = 1), a band's wrapped frame
 * columns included:
 *   CUM_DOTRAN  2-D, 0 or 1
 *   CUM_KTOP    2-D, kcumtop as doubles holding integers in 0 .. kz (like KPBL)
 *   CUM_CLDFRA  kz levels, convcldfra, finite and in [0, 1]
 * A value outside those sets refuses the whole put.  A put writes the buffers the captured graphs
 * read: it drops nothing.  Both fail while the switch is off and for an unknown field. */
enum rcmdyn_cumtran_field { RCMDYN_CUM_DOTRAN = 0, RCMDYN_CUM_KTOP, RCMDYN_CUM_CLDFRA, RCMDYN_NCUMFIELDS };
int rcmdyn_set_cumtran(rcmdyn_t* h, int32_t on, int32_t ncum);
int rcmdyn_put_cumtran(rcmdyn_t* h, int32_t field, const double* src,
                       int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
int rcmdyn_get_cumtran(rcmdyn_t* h, int32_t field, double* dst,
                       int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);

/* Tracer budget (the reference's ichdiag > 0): the accumulators of the five ten2diag calls on
 * aten%chi (Main/mod_tendency.F90:1403-1412, 1503-1511, 1540-1542) and of cumtran (Main/chemlib/
 * mod_che_cumtran.F90:124-130, 159-166), kz levels per tracer, on the interior cross points:
 *   TRDIAG_ADVH  cadvhdiag += chidyn * rw after hadv (the running sum is 0 + hadv)
 *   TRDIAG_ADVV  cadvvdiag += (chidyn after vadv - after hadv) * rw
 *   TRDIAG_BDY   cbdydiag  += (after nudge_chi - before) * rw; booked on every iboudy, + 0.0 where
 *                nothing is relaxed (iboudy other than 1 / 5, or zero tables)
 *   TRDIAG_DIFH  cdifhdiag += (after diffu_x - before) * rw
 *   TRDIAG_CONV  cconvdiag += (atm2 after cumtran - before) / dt * 2 * cfdout, in a tend where
 *                cumtran acts (with cumtran off it stays zero)
 * Each stage term is the rounded difference of two running sums times rw, then added, as
 * extracttenchi forms it (:2177-2207).  rw is alarm_out_atm%rw, cfdout alarm_out_che%rw
 * (Main/chemlib/mod_che_start.F90:341).  The prognostic results are identical with the budget on
 * or off.  The boundary-layer, convection-scheme, emission, deposition and chemistry diagnostics
 * (ctbldiag, the scheme's own cconvdiag share, ...) stay the host's.
 *
 * rcmdyn_set_tracer_budget: refused without tracers and for a non-finite factor.  The switch or a
 * changed factor drops the captured graphs, as rcmdyn_set_budget does; the sums start at zero at
 * a switch-on from off.  rcmdyn_set_tracers with another count switches it off and frees it.
 * rcmdyn_get_tracer_budget: one term (enum rcmdyn_tracer_diag) of tracer itr = 1..ntr, box rules
 * as rcmdyn_get_budget; refused while off and for a term or itr out of range.
 * rcmdyn_reset_tracer_budget: zeroes every sum (the host does it after writing them at
 * alarm_out_che).  There is no put: the reference does not carry the sums through SAV. */
enum rcmdyn_tracer_diag {
  RCMDYN_TRDIAG_ADVH = 0, RCMDYN_TRDIAG_ADVV, RCMDYN_TRDIAG_BDY, RCMDYN_TRDIAG_DIFH, RCMDYN_TRDIAG_CONV,
  RCMDYN_NTRDIAG
};
int rcmdyn_set_tracer_budget(rcmdyn_t* h, int32_t on, double rw, double cfdout);
int rcmdyn_get_tracer_budget(rcmdyn_t* h, int32_t term, int32_t itr, double* dst,
                             int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);
int rcmdyn_reset_tracer_budget(rcmdyn_t* h);

/* Device output stream: the dyn-owned fields of mod_output's ATM stream and the dyn-owned parts of
 * SRF / SHF (Main/mod_output.F90:224-660, 923-1154), formed on the device from the state as it
 * stands at the call, written compact over each tile's own jci1:jci2 x ici1:ici2 in fp64 or fp32
 * (the stream files store 4-byte reals) and handed to the host without stalling later steps.  Off
 * by default and outside the captured step: with the stage off no launch of it is issued.  Every
 * expression is the reference's, in its order; the fp32 form is one (float) rounding of the
 * finished fp64 value.  The lines cited define each field (idynamic 1 and 2):
 *   OUT_PS      :226   sfs%psa (cb)
 *   OUT_PS_PA   :933-941  surface pressure in Pa (NH: atm0%ps + ptop * 1000 + pp(kz) / psa)
 *   OUT_T       :234
 *   OUT_U, OUT_V  :255-258, the four-point dot -> cross mean over psa, with the ghost line of
 *               atm1%u, atm1%v the reference exchanges at :250-251
 *   OUT_W       :277   NH only
 *   OUT_PP      :291   NH only
 *   OUT_QV      :301, :305  specific humidity
 *   OUT_QC, OUT_QI, OUT_QR, OUT_QS  :314, :336, :325, :347; the last three with nqx = 5 only
 *   OUT_TKE     :576   levels 1..kz, ibltyp = 2 only
 *   OUT_PH      :388 (the full-level sigma(k), as the text has it), NH :409-414
 *   OUT_ZH      :396-403, hydrostatic only (the NH value is the constant atm0%z the host holds)
 *   OUT_UA100, OUT_VA100  :1057-1150 (2-D): the hydrostatic branch rebuilds its heights from the
 *               current state, the NH branch reads ATM0_Z; a column with no half level above
 *               100 m gets zero (the text's loop leaves the stream buffer's previous record)
 *   OUT_RH      :366-368 (percent)
 *   OUT_PF      :378
 *   OUT_ZF      :452   hydrostatic only
 *   OUT_OMEGA   :268   RCMDYN_OMEGA * 10 (hPa/s), hydrostatic only: the NH step does not fill that
 *               export (the host has the NH omega in ATMS_WPX3D)
 * Leftover fields.  When output runs after a step, atm1%pr (Main/mod_tendency.F90:1038, 1057),
 * atms%zq, atms%pf3d (mkslice) and omega still hold what the last tend left at its start, so
 * OUT_RH, OUT_PF, OUT_ZF and levels 1..kz-1 of OUT_ZH mix new and old state (:400 adds the old
 * zq(k+1) to a layer built from the new t); the engine reproduces that mix.  They are served from
 * the mkslice export of the last rcmdyn_tend_pre_physics issued with the stage on (which then also
 * keeps atm1%pr) and are refused with the slice fields' 'no slice fields yet' message until then: in
 * a job stepping with rcmdyn_step only, and at lcount = 0, the host still holds its own values.
 * OUT_OMEGA is refused while rcmdyn_set_diagnostics is off.  A field the configuration lacks is
 * refused by name.
 * Left on the host: uvrotate (wind_antirotate has one branch per projection; the host applies it
 * to the fetched u, v), CAPE / CIN (getcape), every physics-owned variable of the streams, the
 * idiag terms (rcmdyn_get_budget serves them) and NetCDF itself. */
enum rcmdyn_output_field {
  RCMDYN_OUT_PS = 0, RCMDYN_OUT_PS_PA, RCMDYN_OUT_T, RCMDYN_OUT_U, RCMDYN_OUT_V, RCMDYN_OUT_W, RCMDYN_OUT_PP,
  RCMDYN_OUT_QV, RCMDYN_OUT_QC, RCMDYN_OUT_QI, RCMDYN_OUT_QR, RCMDYN_OUT_QS, RCMDYN_OUT_TKE, RCMDYN_OUT_PH,
  RCMDYN_OUT_ZH, RCMDYN_OUT_UA100, RCMDYN_OUT_VA100, RCMDYN_OUT_RH, RCMDYN_OUT_PF, RCMDYN_OUT_ZF,
  RCMDYN_OUT_OMEGA,
  RCMDYN_NOUT
};
/* rcmdyn_set_output: prec is 4 (float) or 8 (double), refused otherwise with the switch as it was.
 * The first switch-on allocates the compact device buffers and the pinned host buffers.  The step
 * graphs are not touched.  A switch or a changed prec forgets the last snapshot.
 * rcmdyn_output_atm: mask has bit (1 << field) set for every requested field.  Settles a lazy tend,
 * exchanges the 1-deep ghost line of atm1%u, atm1%v where tiles or a period need it (collective
 * over the ranks of a job, like rcmdyn_reductions: every rank calls it with the same mask), forms
 * the fields in one launch per tile on the compute stream and starts the device -> pinned copy on
 * a copy stream behind it, then returns without waiting.  A second call first waits for the
 * previous copy.  Refused, with nothing launched, while the stage is off, for an empty mask or an
 * unknown bit, and for a field that is refused (above).
 * rcmdyn_get_output: one field of the last rcmdyn_output_atm into dst (floats or doubles by prec),
 * layout and global bounds as in rcmdyn_get (2-D fields with k1 = k2 = 1); only the interior
 * cross points of the owned tiles that lie in the box are written.  Waits for that copy only,
 * never for steps issued after rcmdyn_output_atm; a failure of a step issued before it is
 * reported as rcmdyn_get does.  Refused for a field that was not in the last mask. */
int rcmdyn_set_output(rcmdyn_t* h, int32_t on, int32_t prec);
int rcmdyn_output_atm(rcmdyn_t* h, uint32_t mask);
int rcmdyn_get_output(rcmdyn_t* h, int32_t field, void* dst,
                      int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);

/* Device output stream of the tracers: the fields of the CHE file that the dyn core owns
 * (fill_chem_outvars, Main/chemlib/mod_che_output.F90), formed on the device per tracer, written
 * compact over each tile's own jci1:jci2 x ici1:ici2 in fp64 or fp32 and handed to the host without
 * stalling later steps.  Off by default and outside the captured step: with the stage off no launch
 * of it is issued.  The fp32 form is one (float) rounding of the finished fp64 value.  The lines
 * cited define each field (idynamic 1 and 2, the idynamic /= 3 branch):
 *   CHE_MIXRAT  :74-79    chia(j,i,k,itr) / cpsb(j,i), kz levels; cpsb is sfs%psb
 *               (Main/mod_che_interface.F90:128); a division, not a product with a reciprocal
 *   CHE_BURDEN  :81-83    dtrace(j,i,itr) * 1.0e6, 2-D; dtrace is Main/chemlib/mod_che_tend.F90:561-571:
 *               from zero, over k = 1 .. kz in that order, dtrace + chib3d * cdzq * crhob3d (left to
 *               right, no contraction).  cdzq is atms%dzq: mkslice's on the hydrostatic core
 *               (ATMS_DZQ), the constant atm0%dzf = atm0%zf(k) - atm0%zf(k+1) on the NH core
 *               (Main/mod_atm_interface.F90:977, Main/mod_params.F90:2636; from ATM0_ZF)
 *   CHE_ADVH, CHE_ADVV, CHE_BDY, CHE_DIFH, CHE_CONV  :131-158, 178-184  the accumulator of the same
 *               name of enum rcmdyn_tracer_diag divided by cpsb, kz levels.  CHE_CONV is the
 *               device's share (cumtran): the host adds its cumulus scheme's share itself.
 * Leftover field.  The reference forms dtrace inside the last tend's physics call, so CHE_BURDEN
 * is served from the mkslice export of the last rcmdyn_tend_pre_physics (TR_CHIB3D, ATMS_DZQ,
 * ATMS_RHOB3D) and is refused with the slice fields' 'no slice fields yet' message until then.
 * The five budget fields are refused by name while the tracer budget is off.
 * Read-and-zero.  fill_chem_outvars zeroes every c*diag(:,:,:,itr) whenever ichdiag > 0, whether
 * or not the variable is written: with the tracer budget on, rcmdyn_output_che zeroes all five sums
 * of every tracer in itr1..itr2 in the kernel pass that reads them, whatever the mask.  The sums of
 * the tracers outside the range are untouched.  The pass sits on the compute stream in issue order:
 * steps issued afterwards accumulate from zero.  With the budget off nothing is zeroed.
 *
 * rcmdyn_set_output_che: prec is 4 (float) or 8 (double); nbatch (1 .. ntr) is the largest number
 * of tracers one rcmdyn_output_che takes and sizes the buffers: two sets of a compact device
 * buffer and a pinned host buffer per tile, each with room for all RCMDYN_NCHE fields of nbatch
 * tracers.  Refused, with the switch as it was, without tracers and for a prec or nbatch out of
 * range.  A switch or a changed prec / nbatch forgets both snapshots; switching off frees the
 * buffers; rcmdyn_set_tracers with another count switches the stage off and frees them.  The step
 * graphs are not touched.
 * rcmdyn_output_che: mask has bit (1 << field) set for every requested field; the tracers are
 * itr1 .. itr2 (from 1), at most nbatch of them.  Settles a lazy tend, forms the fields in one
 * launch per tile on the compute stream into the buffer set that is not the previous call's, and
 * starts its device -> pinned copy, with the step's sticky error flags of that moment, on a copy
 * stream behind an event; returns without waiting.  A call waits only for the copy issued two
 * calls back, so the host can issue batch b + 1 before it fetches and writes batch b
 * (Main/mod_output.F90:1379-1382 writes the record one tracer at a time).  No exchange: every
 * input is read at the thread's own point; every rank owns its tiles.  Refused, with nothing
 * launched and nothing zeroed, while the stage is off, for an empty mask or an unknown bit, for
 * itr1 < 1, itr2 > ntr, itr1 > itr2 or more than nbatch tracers, and for a field that is refused
 * (above).
 * rcmdyn_get_output_che: one field of one tracer into dst (floats or doubles by prec), layout and
 * global bounds as in rcmdyn_get (CHE_BURDEN with k1 = k2 = 1); only the interior cross points of
 * the owned tiles that lie in the box are written.  Serves the newer of the two held snapshots
 * that holds itr with field in its mask and waits for that snapshot's copy only, never for steps
 * issued after it; a failure of a step issued before it is reported as rcmdyn_get does.  Refused
 * for a field or tracer that neither held snapshot has.
 * The copy stream is the stage's own, not rcmdyn_output_atm's, so a long CHE batch does not hold
 * back a short ATM record.  The two stages cannot wait on each other: each copy stream waits only
 * for an event recorded on the compute stream, the compute stream waits for neither copy stream,
 * and the host waits only for copy events that are already recorded. */
enum rcmdyn_che_field {
  RCMDYN_CHE_MIXRAT = 0, RCMDYN_CHE_BURDEN, RCMDYN_CHE_ADVH, RCMDYN_CHE_ADVV, RCMDYN_CHE_BDY, RCMDYN_CHE_DIFH,
  RCMDYN_CHE_CONV,
  RCMDYN_NCHE
};
int rcmdyn_set_output_che(rcmdyn_t* h, int32_t on, int32_t prec, int32_t nbatch);
int rcmdyn_output_che(rcmdyn_t* h, uint32_t mask, int32_t itr1, int32_t itr2);
int rcmdyn_get_output_che(rcmdyn_t* h, int32_t field, int32_t itr, void* dst,
                          int32_t j1, int32_t j2, int32_t i1, int32_t i2, int32_t k1, int32_t k2);

/* Per-kernel device time (measurement hook, mirrors rocprofv3 --kernel-trace --stats):
 * runs nsteps steps (tend + bdyval, eagerly, no graph) with a HIP event pair around every
 * kernel launch on the engine's stream.  For each distinct kernel (at most cap) fills
 * names[q*48 .. q*48+47] (NUL-terminated), launches[q] and avg_ms[q] (mean duration per
 * launch); *count = kernels found.  The steps advance the model like rcmdyn_step. */
int rcmdyn_kernel_times(rcmdyn_t* h, int32_t nsteps, int32_t cap, char* names, int32_t* launches,
                        double* avg_ms, int32_t* count);

#ifdef __cplusplus
}
#endif
#endif /* RCMDYN_H */
