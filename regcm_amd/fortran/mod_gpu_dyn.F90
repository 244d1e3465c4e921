!
! mod_gpu_dyn -- Fortran 2003 ISO_C_BINDING shim over the rcmdyn C-ABI (include/rcmdyn.h).
!
! This is the module a RegCM 4.7 host links to run the dynamical-core step on MI355X
! instead of `call tend` / `call bdyval` (Main/mod_regcm_interface.F90:189,208).  Arrays are
! passed with their Fortran bounds exactly as getmem* allocated them (j fastest), so the
! host keeps its own layout and never sees device memory.  See INTEGRATION.md.
!
module mod_gpu_dyn
  use iso_c_binding
  implicit none
  private

  integer, parameter, public :: rcmdyn_abi_version = 6
  integer, parameter, public :: rcmdyn_maxkz = 64, rcmdyn_maxsplit = 4

  ! field ids (enum rcmdyn_field)
  integer(c_int32_t), parameter, public :: &
    f_atm1_u = 0, f_atm1_v = 1, f_atm1_t = 2, f_atm1_qv = 3, f_atm1_qc = 4, &
    f_atm2_u = 5, f_atm2_v = 6, f_atm2_t = 7, f_atm2_qv = 8, f_atm2_qc = 9, &
    f_psa = 10, f_psb = 11, f_dstor = 12, f_hstor = 13, &
    f_msfx = 14, f_msfd = 15, f_coriol = 16, f_ht = 17, &
    f_xub_b0 = 18, f_xub_bt = 19, f_xvb_b0 = 20, f_xvb_bt = 21, f_xtb_b0 = 22, &
    f_xtb_bt = 23, f_xqb_b0 = 24, f_xqb_bt = 25, f_xpsb_b0 = 26, f_xpsb_bt = 27, &
    f_psc = 28, f_pten = 29, f_psdota = 30, f_tten = 31, f_uten = 32, f_vten = 33, &
    f_qvten = 34, f_qcten = 35, f_omega = 36, f_qdot = 37, f_xkc = 38, f_phi = 39, &
    f_atm1_pp = 40, f_atm2_pp = 41, f_atm1_w = 42, f_atm2_w = 43, &
    f_xppb_b0 = 44, f_xppb_bt = 45, f_xwwb_b0 = 46, f_xwwb_bt = 47, &
    f_atm0_ps = 48, f_atm0_pr = 49, f_atm0_t = 50, f_atm0_rho = 51, f_atm0_z = 52, &
    f_atm0_pf = 53, f_atm0_rhof = 54, f_atm0_zf = 55, f_dpsdxm = 56, f_dpsdym = 57, &
    f_dprddx = 58, f_dprddy = 59, f_ef = 60, f_ddx = 61, f_ddy = 62, f_dmdx = 63, &
    f_dmdy = 64, f_ex = 65, f_crx = 66, f_cry = 67, &
    ! physics coupling seam: pc_physic tendencies (put) and the mkslice export (get)
    f_tphy = 68, f_qvphy = 69, f_qcphy = 70, f_uphy = 71, f_vphy = 72, f_ppphy = 73, f_wphy = 74, &
    f_atms_ubx3d = 75, f_atms_vbx3d = 76, f_atms_ubd3d = 77, f_atms_vbd3d = 78, f_atms_tb3d = 79, &
    f_atms_qvb3d = 80, f_atms_qcb3d = 81, f_atms_tv3d = 82, f_atms_pb3d = 83, f_atms_pf3d = 84, &
    f_atms_ps2d = 85, f_atms_rhox2d = 86, f_atms_th3d = 87, f_atms_rhob3d = 88, f_atms_tp3d = 89, &
    f_atms_wpx3d = 90, f_atms_wb3d = 91, f_atms_zq = 92, f_atms_za = 93, f_atms_dzq = 94, &
    f_atms_qsb3d = 95, f_atms_rhb3d = 96, &
    ! device bdyin: the next ICBC record as read_icbc returns it; NH atm0%psdot
    f_xub_b1 = 97, f_xvb_b1 = 98, f_xtb_b1 = 99, f_xqb_b1 = 100, f_xpsb_b1 = 101, &
    f_xppb_b1 = 102, f_xwwb_b1 = 103, f_atm0_psdot = 104, &
    f_atm1_tke = 105, f_atm2_tke = 106, f_tkephy = 107, f_kpbl = 108, &
    ! nqx = 5 (ipptls >= 2): atm1/atm2 qx(:,:,:,iqi|iqr|iqs), their qxphy, the qxb3d export
    f_atm1_qi = 109, f_atm1_qr = 110, f_atm1_qs = 111, f_atm2_qi = 112, f_atm2_qr = 113, &
    f_atm2_qs = 114, f_qiphy = 115, f_qrphy = 116, f_qsphy = 117, &
    f_atms_qxb3d_qi = 118, f_atms_qxb3d_qr = 119, f_atms_qxb3d_qs = 120

  ! tendency budget terms of t and qv (enum rcmdyn_budget_term; the reference's idiag = 1:
  ! tdiag / qdiag %adh, adv, adi, bdy, dif) and the species the budget of qv follows
  integer(c_int32_t), parameter, public :: &
    bud_t_adh = 0, bud_t_adv = 1, bud_t_adi = 2, bud_t_bdy = 3, bud_t_dif = 4, &
    bud_q_adh = 5, bud_q_adv = 6, bud_q_adi = 7, bud_q_bdy = 8, bud_q_dif = 9, &
    rcmdyn_nbudget = 10

  ! terms of rcmdyn_get_condtq (enum rcmdyn_condtq_term): the held rh0adj, the last tend's coupled
  ! condensation increments of t, qv, qc (aten(.., pc_physic) after condtq: tdiag%lsc, qdiag%lsc)
  integer(c_int32_t), parameter, public :: &
    condtq_rh0adj = 0, condtq_t = 1, condtq_qv = 2, condtq_qc = 3, rcmdyn_ncondtq = 4

  ! fields of rcmdyn_put_subex / rcmdyn_get_subex (enum rcmdyn_subex_field): the host's 2-D tables,
  ! cucloud's output, the accumulators, and what the device forms (remrat / rembc with rem = 1)
  integer(c_int32_t), parameter, public :: &
    subex_rh0 = 0, subex_qck1 = 1, subex_cgul = 2, subex_cevap = 3, subex_caccr = 4, &
    subex_cu_cldfra = 5, subex_cu_cldlwc = 6, subex_rainnc = 7, subex_lsmrnc = 8, &
    subex_fcc = 9, subex_cldfra = 10, subex_cldlwc = 11, subex_rh0adj = 12, &
    subex_lsc_t = 13, subex_lsc_qv = 14, subex_lsc_qc = 15, subex_trrate = 16, &
    subex_remrat = 17, subex_rembc = 18, rcmdyn_nsubex = 19

  ! fields of one chemical tracer (enum rcmdyn_tracer_field): chia, chib, chiphy (put only), chib0,
  ! chibt, the mkslice export chib3d (get only); the most tracers of one engine (RCMDYN_MAXTR)
  integer(c_int32_t), parameter, public :: &
    tr_atm1 = 0, tr_atm2 = 1, tr_phy = 2, tr_b0 = 3, tr_bt = 4, tr_chib3d = 5, rcmdyn_ntrfields = 6
  integer, parameter, public :: rcmdyn_maxtr = 96

  ! inputs of the tracers' cumulus mixing (enum rcmdyn_cumtran_field): init_cumtran's mask (0 / 1),
  ! kcumtop (both 2-D), convcldfra; terms of the tracer budget (enum rcmdyn_tracer_diag): cadvhdiag,
  ! cadvvdiag, cbdydiag, cdifhdiag, cumtran's share of cconvdiag
  integer(c_int32_t), parameter, public :: &
    cum_dotran = 0, cum_ktop = 1, cum_cldfra = 2, rcmdyn_ncumfields = 3
  integer(c_int32_t), parameter, public :: &
    trdiag_advh = 0, trdiag_advv = 1, trdiag_bdy = 2, trdiag_difh = 3, trdiag_conv = 4, rcmdyn_ntrdiag = 5

  ! fields of the output stream (enum rcmdyn_output_field): the dyn-owned variables of mod_output's
  ! ATM, SRF and SHF streams; rcmdyn_output_atm takes ibset(0, out_x) of every requested one
  integer(c_int32_t), parameter, public :: &
    out_ps = 0, out_ps_pa = 1, out_t = 2, out_u = 3, out_v = 4, out_w = 5, out_pp = 6, out_qv = 7, &
    out_qc = 8, out_qi = 9, out_qr = 10, out_qs = 11, out_tke = 12, out_ph = 13, out_zh = 14, &
    out_ua100 = 15, out_va100 = 16, out_rh = 17, out_pf = 18, out_zf = 19, out_omega = 20, rcmdyn_nout = 21

  ! fields of the tracers' output stream (enum rcmdyn_che_field): the dyn-owned variables of the CHE
  ! file, per tracer; rcmdyn_output_che takes ibset(0, che_x) of every requested one
  integer(c_int32_t), parameter, public :: &
    che_mixrat = 0, che_burden = 1, che_advh = 2, che_advv = 3, che_bdy = 4, che_difh = 5, che_conv = 6, &
    rcmdyn_nche = 7

  type, bind(c), public :: rcmdyn_config
    integer(c_int32_t) :: abi_version
    integer(c_int32_t) :: jx, iy, kz
    integer(c_int32_t) :: nproc_j, nproc_i
    integer(c_int32_t) :: tile_first, tile_count
    integer(c_int32_t) :: idynamic, iboudy, idiffu, ipgf, nsplit, nspgx, nspgd
    integer(c_int32_t) :: diffu_hgtf, upstream_mode, stability_enhance, present_qc
    real(c_double) :: ds, dtsec, ptop, gnu1, gnu2, uoffc, t_extrema, q_rel_extrema
    real(c_double) :: ckh, adyndif, high_nudge, medium_nudge, low_nudge
    real(c_double) :: bdy_nm, bdy_dm, dtbdys
    real(c_double) :: sigma(rcmdyn_maxkz+1)
    real(c_double) :: zmatx(rcmdyn_maxkz,rcmdyn_maxsplit)   ! zmatx(k,l)
    real(c_double) :: zmatxr(rcmdyn_maxkz,rcmdyn_maxsplit)  ! zmatxr(l,k) stored (k,l)
    real(c_double) :: am(rcmdyn_maxkz,rcmdyn_maxsplit)      ! am(k,l)
    real(c_double) :: tau(rcmdyn_maxkz,rcmdyn_maxsplit)     ! tau(l,k) stored (k,l)
    real(c_double) :: varpa1(rcmdyn_maxkz+1,rcmdyn_maxsplit)! varpa1(l,k) stored (k,l)
    real(c_double) :: an(rcmdyn_maxsplit), hbar(rcmdyn_maxsplit)
    real(c_double) :: aam(rcmdyn_maxsplit), dtau(rcmdyn_maxsplit)
    real(c_double) :: sigmah(rcmdyn_maxkz+1)
    real(c_double) :: pd
    integer(c_int32_t) :: comm_rank, comm_size, device
    integer(c_int8_t) :: comm_unique_id(128)
    ! non-hydrostatic core (nonhydroparam, init_sound outputs)
    integer(c_int32_t) :: ifupr, ifrayd, rayndamp, nh_reserved
    real(c_double) :: nhbet, nhxkd, rayalpha0, rayhd, nh_dtsmax, nh_xmsf
    ! cldparam rhmin, rhmax (mkslice rhb3d clamps)
    real(c_double) :: rhmin, rhmax
    ! physicsparam isladvec, iqmsl (semi-Lagrangian moisture advection)
    integer(c_int32_t) :: isladvec, iqmsl
    ! physicsparam ibltyp (2 = UW PBL TKE in the dyn step), uwparam iuwvadv, nuk, tkemin (uwtkemin)
    integer(c_int32_t) :: ibltyp, iuwvadv
    real(c_double) :: nuk, tkemin
    ! ABI 6: physicsparam ipptls and the nqx param sets from it (2, or 5 for ipptls >= 2);
    ! i_band (1: tropical band, hydrostatic core), i_crm, ichem (refused if set: the tracers
    ! are declared with rcmdyn_set_tracers)
    integer(c_int32_t) :: ipptls, nqx
    integer(c_int32_t) :: i_band, i_crm, ichem
  end type rcmdyn_config

  interface
    integer(c_int) function rcmdyn_create(cfg, h) bind(c, name='rcmdyn_create')
      import :: c_int, c_ptr, rcmdyn_config
      type(rcmdyn_config), intent(in) :: cfg
      type(c_ptr), intent(out) :: h
    end function
    integer(c_int) function rcmdyn_destroy(h) bind(c, name='rcmdyn_destroy')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    type(c_ptr) function rcmdyn_last_error(h) bind(c, name='rcmdyn_last_error')
      import :: c_ptr
      type(c_ptr), value :: h
    end function
    integer(c_int) function rcmdyn_put(h, f, src, j1, j2, i1, i2, k1, k2) bind(c, name='rcmdyn_put')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: f, j1, j2, i1, i2, k1, k2
      real(c_double), intent(in) :: src(*)
    end function
    integer(c_int) function rcmdyn_get(h, f, dst, j1, j2, i1, i2, k1, k2) bind(c, name='rcmdyn_get')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: f, j1, j2, i1, i2, k1, k2
      real(c_double), intent(out) :: dst(*)
    end function
    integer(c_int) function rcmdyn_set_time(h, lcount, dt, xbctime) bind(c, name='rcmdyn_set_time')
      import :: c_int, c_ptr, c_int64_t, c_double
      type(c_ptr), value :: h
      integer(c_int64_t), value :: lcount
      real(c_double), value :: dt, xbctime
    end function
    integer(c_int) function rcmdyn_get_time(h, lcount, dt, xbctime) bind(c, name='rcmdyn_get_time')
      import :: c_int, c_ptr, c_int64_t, c_double
      type(c_ptr), value :: h
      integer(c_int64_t), intent(out) :: lcount
      real(c_double), intent(out) :: dt, xbctime
    end function
    integer(c_int) function rcmdyn_tend(h) bind(c, name='rcmdyn_tend')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    integer(c_int) function rcmdyn_tend_pre_physics(h) bind(c, name='rcmdyn_tend_pre_physics')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    integer(c_int) function rcmdyn_tend_post_physics(h) bind(c, name='rcmdyn_tend_post_physics')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    integer(c_int) function rcmdyn_bdyin(h) bind(c, name='rcmdyn_bdyin')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    integer(c_int) function rcmdyn_bdyval(h) bind(c, name='rcmdyn_bdyval')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    integer(c_int) function rcmdyn_step(h, n) bind(c, name='rcmdyn_step')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: n
    end function
    ! the 3-hourly report sums (sumall/maxall over the job): ptntot, pt2tot, NH max CFL
    integer(c_int) function rcmdyn_reductions(h, out) bind(c, name='rcmdyn_reductions')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: out(3)
    end function
    integer(c_int) function rcmdyn_diagnostics(h, out) bind(c, name='rcmdyn_diagnostics')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: out(4)
    end function
    integer(c_int) function rcmdyn_comm_unique_id(out) bind(c, name='rcmdyn_comm_unique_id')
      import :: c_int, c_int8_t
      integer(c_int8_t), intent(out) :: out(128)
    end function
    ! waits for the device and reports any failed step; COLLECTIVE in RCCL mode (every rank
    ! calls it, as every rank calls rcmdyn_step)
    integer(c_int) function rcmdyn_synchronize(h) bind(c, name='rcmdyn_synchronize')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    ! set_nproc (Main/mpplib/mod_mppparam.F90:1053-1371), host-only: cpus = (cpus_j, cpus_i)
    integer(c_int) function rcmdyn_set_nproc(nproc, jx, iy, cpus) bind(c, name='rcmdyn_set_nproc')
      import :: c_int, c_int32_t
      integer(c_int32_t), value :: nproc, jx, iy
      integer(c_int32_t), intent(out) :: cpus(2)
    end function
    ! ext = (jde1,jde2,ide1,ide2,jce1,jce2,ice1,ice2), bdy = (left,right,bottom,top), host-only
    integer(c_int) function rcmdyn_tile_extent(jx, iy, nproc_j, nproc_i, tile, ext, bdy) &
        bind(c, name='rcmdyn_tile_extent')
      import :: c_int, c_int32_t
      integer(c_int32_t), value :: jx, iy, nproc_j, nproc_i, tile
      integer(c_int32_t), intent(out) :: ext(8), bdy(4)
    end function
    ! the same for cfg's grid and decomposition with its periodic directions (i_band: j,
    ! i_crm: i), as the engine's tiles are cut; host-only
    integer(c_int) function rcmdyn_tile_extent_cfg(cfg, tile, ext, bdy) bind(c, name='rcmdyn_tile_extent_cfg')
      import :: c_int, c_int32_t, rcmdyn_config
      type(rcmdyn_config), intent(in) :: cfg
      integer(c_int32_t), value :: tile
      integer(c_int32_t), intent(out) :: ext(8), bdy(4)
    end function
    ! the communication calls of one rank (7 int64 per record), host-only
    integer(c_int) function rcmdyn_exchange_plan(cfg, nsteps, ops, cap, count) bind(c, name='rcmdyn_exchange_plan')
      import :: c_int, c_int32_t, c_int64_t, rcmdyn_config
      type(rcmdyn_config), intent(in) :: cfg
      integer(c_int32_t), value :: nsteps
      integer(c_int64_t), intent(out) :: ops(*)
      integer(c_int64_t), value :: cap
      integer(c_int64_t), intent(out) :: count
    end function
    ! per tile, the points of the update kernels that run beside the prologue exchange
    integer(c_int) function rcmdyn_overlap_shares(cfg, out, cap) bind(c, name='rcmdyn_overlap_shares')
      import :: c_int, c_int32_t, rcmdyn_config
      type(rcmdyn_config), intent(in) :: cfg
      integer(c_int32_t), intent(out) :: out(*)
      integer(c_int32_t), value :: cap
    end function
    ! the HIP runtime and librccl the engine is bound to (a NUL-terminated string)
    integer(c_int) function rcmdyn_runtime_info(buf, len) bind(c, name='rcmdyn_runtime_info')
      import :: c_int, c_char, c_int32_t
      character(kind=c_char), intent(out) :: buf(*)
      integer(c_int32_t), value :: len
    end function
    ! average device ms per step of the last rcmdyn_step call
    integer(c_int) function rcmdyn_last_step_ms(h, ms) bind(c, name='rcmdyn_last_step_ms')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: ms
    end function
    ! the per-point tendency diagnostics (f_tten .. f_xkc) on (1) or off (0, the default)
    integer(c_int) function rcmdyn_set_diagnostics(h, on) bind(c, name='rcmdyn_set_diagnostics')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on
    end function
    ! the tendency budget of t and qv on (1) or off (0, the default); idgq must be iqv, rw is
    ! alarm_out_atm%rw
    integer(c_int) function rcmdyn_set_budget(h, on, idgq, rw) bind(c, name='rcmdyn_set_budget')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on, idgq
      real(c_double), value :: rw
    end function
    ! one accumulator (bud_t_adh .. bud_q_dif) into dst(j1:j2,i1:i2,k1:k2)
    integer(c_int) function rcmdyn_get_budget(h, term, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_budget')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: term, j1, j2, i1, i2, k1, k2
      real(c_double), intent(out) :: dst(*)
    end function
    ! zeroes the ten accumulators (after the host wrote them to the ATM file)
    integer(c_int) function rcmdyn_reset_budget(h) bind(c, name='rcmdyn_reset_budget')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    ! the mass check of tend (Main/mod_massck.F90) on (1) or off (0, the default), with a device
    ! log of cap records (1..65536)
    integer(c_int) function rcmdyn_set_massck(h, on, cap) bind(c, name='rcmdyn_set_massck')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on, cap
    end function
    ! the records since the last call into recs(6,cap), oldest first: lcount, dt, drymass,
    ! dryadv, qmass, qadv; count of them copied, lost older ones; collective over the ranks
    integer(c_int) function rcmdyn_get_massck(h, recs, cap, count, lost) bind(c, name='rcmdyn_get_massck')
      import :: c_int, c_ptr, c_int32_t, c_int64_t, c_double
      type(c_ptr), value :: h
      real(c_double), intent(out) :: recs(*)
      integer(c_int32_t), value :: cap
      integer(c_int32_t), intent(out) :: count
      integer(c_int64_t), intent(out) :: lost
    end function
    ! the SUBEX condensation (condtq, ipptls = 1) inside tend on (1) or off (0, the default); conf
    ! is subexparam's condensation efficiency, in (0, 1]
    integer(c_int) function rcmdyn_set_condtq(h, on, conf) bind(c, name='rcmdyn_set_condtq')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on
      real(c_double), value :: conf
    end function
    ! cldfrac's rh0adj(j1:j2,i1:i2,k1:k2), every value in [0, 0.99999]; on the split path between
    ! rcmdyn_tend_pre_physics and rcmdyn_tend_post_physics.  tend waits for one put since the
    ! switch-on that covers the tiles' interior cross points and their rings on every level
    integer(c_int) function rcmdyn_put_rh0adj(h, src, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_put_rh0adj')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: src(*)
      integer(c_int32_t), value :: j1, j2, i1, i2, k1, k2
    end function
    ! one term (condtq_rh0adj .. condtq_qc) into dst(j1:j2,i1:i2,k1:k2)
    integer(c_int) function rcmdyn_get_condtq(h, term, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_condtq')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: term, j1, j2, i1, i2, k1, k2
      real(c_double), intent(out) :: dst(*)
    end function
    ! SUBEX on the device (ipptls = 1): cldfrac with subex_cldfrac and the rain columns of subex in
    ! physical_parametrizations' place, on (1) or off (0, the default).  rhmax, rhmin, tc0,
    ! larcticcorr, iconvlwp: the run's settings; rem = 1: also remrat / rembc (ichem = 1).
    ! icldfrac, icldmstrat, lsecind: the host's settings of options that are not built, anything
    ! but 0 is refused by name
    integer(c_int) function rcmdyn_set_subex(h, on, rhmax, rhmin, tc0, larcticcorr, iconvlwp, rem, &
        icldfrac, icldmstrat, lsecind) bind(c, name='rcmdyn_set_subex')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on
      real(c_double), value :: rhmax, rhmin, tc0
      integer(c_int32_t), value :: larcticcorr, iconvlwp, rem, icldfrac, icldmstrat, lsecind
    end function
    ! one field the host owns (subex_rh0 .. subex_lsmrnc) from src(j1:j2,i1:i2,k1:k2); the five
    ! tables must cover the interior cross points before the first run
    integer(c_int) function rcmdyn_put_subex(h, field, src, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_put_subex')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: field
      real(c_double), intent(in) :: src(*)
      integer(c_int32_t), value :: j1, j2, i1, i2, k1, k2
    end function
    ! one field (subex_rainnc .. subex_rembc) into dst(j1:j2,i1:i2,k1:k2), interior cross points
    integer(c_int) function rcmdyn_get_subex(h, field, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_subex')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: field, j1, j2, i1, i2, k1, k2
      real(c_double), intent(out) :: dst(*)
    end function
    ! the subex kernels of the split path, between rcmdyn_tend_pre_physics and
    ! rcmdyn_tend_post_physics (which runs them first if this was not called); once per tend
    integer(c_int) function rcmdyn_physics_subex(h) bind(c, name='rcmdyn_physics_subex')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    ! the chemical tracers (the reference's ichem = 1 chain of tend and bdyval): ntr of them
    ! (0: the family off, its buffers freed); ichebdy must be 1
    integer(c_int) function rcmdyn_set_tracers(h, ntr, ichebdy) bind(c, name='rcmdyn_set_tracers')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: ntr, ichebdy
    end function
    ! one field (tr_atm1 .. tr_bt) of tracer itr = 1..ntr from src(j1:j2,i1:i2,k1:k2)
    integer(c_int) function rcmdyn_put_tracer(h, f, itr, src, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_put_tracer')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: f, itr, j1, j2, i1, i2, k1, k2
      real(c_double), intent(in) :: src(*)
    end function
    ! one field (tr_atm1, tr_atm2, tr_b0, tr_bt, tr_chib3d) of tracer itr into dst(j1:j2,i1:i2,k1:k2)
    integer(c_int) function rcmdyn_get_tracer(h, f, itr, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_tracer')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: f, itr, j1, j2, i1, i2, k1, k2
      real(c_double), intent(out) :: dst(*)
    end function
    ! nudge_chiten's tables cefc(nspgx,kz), cegc(nspgx,kz); zero until put, as the reference leaves them
    integer(c_int) function rcmdyn_put_tracer_nudge(h, cefc, cegc) bind(c, name='rcmdyn_put_tracer_nudge')
      import :: c_int, c_ptr, c_double
      type(c_ptr), value :: h
      real(c_double), intent(in) :: cefc(*), cegc(*)
    end function
    ! cumtran (ichcumtra = 1) inside tend on (1) or off (0, the default); ncum = dtcum / dtsec: it
    ! acts in a tend whose clock has lcount > 0 and mod(lcount, ncum) == 0
    integer(c_int) function rcmdyn_set_cumtran(h, on, ncum) bind(c, name='rcmdyn_set_cumtran')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on, ncum
    end function
    ! one input (cum_dotran, cum_ktop: 2-D, k1 = k2 = 1; cum_cldfra) from src(j1:j2,i1:i2,k1:k2);
    ! the host puts kcumtop and convcldfra after its cumulus call
    integer(c_int) function rcmdyn_put_cumtran(h, f, src, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_put_cumtran')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: f, j1, j2, i1, i2, k1, k2
      real(c_double), intent(in) :: src(*)
    end function
    integer(c_int) function rcmdyn_get_cumtran(h, f, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_cumtran')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: f, j1, j2, i1, i2, k1, k2
      real(c_double), intent(out) :: dst(*)
    end function
    ! the tracer budget (ichdiag > 0) on (1) or off (0, the default); rw = alarm_out_atm%rw,
    ! cfdout = alarm_out_che%rw
    integer(c_int) function rcmdyn_set_tracer_budget(h, on, rw, cfdout) bind(c, name='rcmdyn_set_tracer_budget')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on
      real(c_double), value :: rw, cfdout
    end function
    ! one term (trdiag_advh .. trdiag_conv) of tracer itr into dst(j1:j2,i1:i2,k1:k2)
    integer(c_int) function rcmdyn_get_tracer_budget(h, term, itr, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_tracer_budget')
      import :: c_int, c_ptr, c_int32_t, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: term, itr, j1, j2, i1, i2, k1, k2
      real(c_double), intent(out) :: dst(*)
    end function
    integer(c_int) function rcmdyn_reset_tracer_budget(h) bind(c, name='rcmdyn_reset_tracer_budget')
      import :: c_int, c_ptr
      type(c_ptr), value :: h
    end function
    ! the output stream on (1) or off (0, the default); prec = 4: the host gets reals of 4 bytes,
    ! prec = 8: of 8
    integer(c_int) function rcmdyn_set_output(h, on, prec) bind(c, name='rcmdyn_set_output')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on, prec
    end function
    ! forms the fields of mask (bit out_x per field) from the state as it stands and starts their
    ! copy to the host; does not wait
    integer(c_int) function rcmdyn_output_atm(h, mask) bind(c, name='rcmdyn_output_atm')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: mask
    end function
    ! one field (out_ps .. out_omega) of the last rcmdyn_output_atm into dst(j1:j2,i1:i2,k1:k2), an
    ! array of real(c_float) or real(c_double) by prec, passed as c_loc(dst)
    integer(c_int) function rcmdyn_get_output(h, field, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_output')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: field, j1, j2, i1, i2, k1, k2
      type(c_ptr), value :: dst
    end function
    ! the tracers' output stream on (1) or off (0, the default); prec = 4: the host gets reals of 4
    ! bytes, prec = 8: of 8; nbatch (1 .. ntr): the most tracers one rcmdyn_output_che takes
    integer(c_int) function rcmdyn_set_output_che(h, on, prec, nbatch) bind(c, name='rcmdyn_set_output_che')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: on, prec, nbatch
    end function
    ! forms the fields of mask (bit che_x per field) of the tracers itr1 .. itr2 from the state as it
    ! stands and starts their copy to the host; does not wait.  With the tracer budget on it zeroes
    ! the five sums of these tracers.  The engine holds the snapshots of the last two calls.
    integer(c_int) function rcmdyn_output_che(h, mask, itr1, itr2) bind(c, name='rcmdyn_output_che')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: mask, itr1, itr2
    end function
    ! one field (che_mixrat .. che_conv) of tracer itr from the newer held snapshot that has it into
    ! dst(j1:j2,i1:i2,k1:k2), an array of real(c_float) or real(c_double) by prec, passed as c_loc(dst)
    integer(c_int) function rcmdyn_get_output_che(h, field, itr, dst, j1, j2, i1, i2, k1, k2) &
        bind(c, name='rcmdyn_get_output_che')
      import :: c_int, c_ptr, c_int32_t
      type(c_ptr), value :: h
      integer(c_int32_t), value :: field, itr, j1, j2, i1, i2, k1, k2
      type(c_ptr), value :: dst
    end function
    ! per-kernel device time over nsteps eager steps (names: 48 characters per kernel)
    integer(c_int) function rcmdyn_kernel_times(h, nsteps, cap, names, launches, avg_ms, count) &
        bind(c, name='rcmdyn_kernel_times')
      import :: c_int, c_ptr, c_int32_t, c_char, c_double
      type(c_ptr), value :: h
      integer(c_int32_t), value :: nsteps, cap
      character(kind=c_char), intent(out) :: names(*)
      integer(c_int32_t), intent(out) :: launches(*)
      real(c_double), intent(out) :: avg_ms(*)
      integer(c_int32_t), intent(out) :: count
    end function
  end interface

  public :: rcmdyn_create, rcmdyn_destroy, rcmdyn_put, rcmdyn_get, rcmdyn_set_time
  public :: rcmdyn_get_time, rcmdyn_tend, rcmdyn_bdyval, rcmdyn_step, rcmdyn_diagnostics, rcmdyn_reductions
  public :: rcmdyn_tend_pre_physics, rcmdyn_tend_post_physics, rcmdyn_bdyin, rcmdyn_last_error
  public :: rcmdyn_synchronize, rcmdyn_set_nproc, rcmdyn_tile_extent, rcmdyn_tile_extent_cfg, rcmdyn_exchange_plan
  public :: rcmdyn_overlap_shares, rcmdyn_runtime_info, rcmdyn_last_step_ms, rcmdyn_set_diagnostics
  public :: rcmdyn_kernel_times, rcmdyn_set_budget, rcmdyn_get_budget, rcmdyn_reset_budget
  public :: rcmdyn_set_massck, rcmdyn_get_massck
  public :: rcmdyn_set_condtq, rcmdyn_put_rh0adj, rcmdyn_get_condtq
  public :: rcmdyn_set_subex, rcmdyn_put_subex, rcmdyn_get_subex, rcmdyn_physics_subex
  public :: rcmdyn_set_tracers, rcmdyn_put_tracer, rcmdyn_get_tracer, rcmdyn_put_tracer_nudge
  public :: rcmdyn_set_cumtran, rcmdyn_put_cumtran, rcmdyn_get_cumtran
  public :: rcmdyn_set_tracer_budget, rcmdyn_get_tracer_budget, rcmdyn_reset_tracer_budget
  public :: rcmdyn_set_output, rcmdyn_output_atm, rcmdyn_get_output
  public :: rcmdyn_set_output_che, rcmdyn_output_che, rcmdyn_get_output_che
  public :: rcmdyn_comm_unique_id, gpu_dyn_check, gpu_put3d, gpu_get3d, gpu_put2d, gpu_get2d

  contains

  ! Abort like the reference's fatal() (Share/mod_message.F90:90-103) on any engine error.
  subroutine gpu_dyn_check(h, ierr, where)
    type(c_ptr), intent(in) :: h
    integer(c_int), intent(in) :: ierr
    character(len=*), intent(in) :: where
    character(kind=c_char), pointer :: msg(:)
    integer :: n
    if ( ierr == 0 ) return
    call c_f_pointer(rcmdyn_last_error(h), msg, [1024])
    n = 0
    do while ( n < 1024 )
      if ( msg(n+1) == c_null_char ) exit
      n = n + 1
    end do
    write(0,*) 'mod_gpu_dyn: ', where, ': ', msg(1:n)
    error stop 1
  end subroutine gpu_dyn_check

  ! Put/get a pointer array allocated as a(j1:j2,i1:i2,k1:k2) by getmem3d: pointer
  ! dummies keep the host's lower bounds, which the C-ABI takes as global indices.
  subroutine gpu_put3d(h, f, a)
    type(c_ptr), intent(in) :: h
    integer(c_int32_t), intent(in) :: f
    real(c_double), pointer, contiguous, intent(in) :: a(:,:,:)
    call gpu_dyn_check(h, rcmdyn_put(h, f, a, lbound(a,1), ubound(a,1), lbound(a,2), &
         ubound(a,2), lbound(a,3), ubound(a,3)), 'put3d')
  end subroutine gpu_put3d
  subroutine gpu_get3d(h, f, a)
    type(c_ptr), intent(in) :: h
    integer(c_int32_t), intent(in) :: f
    real(c_double), pointer, contiguous, intent(in) :: a(:,:,:)
    call gpu_dyn_check(h, rcmdyn_get(h, f, a, lbound(a,1), ubound(a,1), lbound(a,2), &
         ubound(a,2), lbound(a,3), ubound(a,3)), 'get3d')
  end subroutine gpu_get3d
  subroutine gpu_put2d(h, f, a)
    type(c_ptr), intent(in) :: h
    integer(c_int32_t), intent(in) :: f
    real(c_double), pointer, contiguous, intent(in) :: a(:,:)
    call gpu_dyn_check(h, rcmdyn_put(h, f, a, lbound(a,1), ubound(a,1), lbound(a,2), &
         ubound(a,2), 1, 1), 'put2d')
  end subroutine gpu_put2d
  subroutine gpu_get2d(h, f, a)
    type(c_ptr), intent(in) :: h
    integer(c_int32_t), intent(in) :: f
    real(c_double), pointer, contiguous, intent(in) :: a(:,:)
    call gpu_dyn_check(h, rcmdyn_get(h, f, a, lbound(a,1), ubound(a,1), lbound(a,2), &
         ubound(a,2), 1, 1), 'get2d')
  end subroutine gpu_get2d

end module mod_gpu_dyn
