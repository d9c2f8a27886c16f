// The magnitude twins of the pulse train's two least-squares walks: k_bloch_train_run_lsq_mag, the text of
// k_bloch_train_run_lsq (blochtraingn_lsq.inc), and k_bloch_train_run_sched_lsq_mag, the text of
// k_bloch_train_run_sched_lsq (blochtrainschedgn_lsq.inc), each with TRAIN_MAG true: per echo and at the final state the
// residual is (rho - t_xy, e_z - t_z) with rho = sqrt(ex ex + ey ey) of the echo as k_bloch_train_run forms it (bloch_mag_dir), the
// cotangent rw_k (w_xy (rho - t_xy) u, w_z (e_z - t_z)) with u = (ex, ey) / rho, zero where rho is 0 (bloch_mag_seed), and the loss
// 1/2 rw_k (w_xy (rho - t_xy)^2 + w_z (e_z - t_z)^2).  Everything else of the walks is their twins'.
// They are compiled here and not beside their twins: a second kernel with the same LDS arrays in blochtraingn.hip or in
// blochtrainschedgn.hip gave the component kernel another LDS layout, and its device code must not change.  The twins of the two
// Gauss-Newton walks (k_bloch_train_run_gn_mag, k_bloch_train_lm_run_mag, k_bloch_train_run_sched_gn_mag,
// k_bloch_train_lm_sched_run_mag) do stand beside theirs, on bodies of sim_dev.h.
#include "dev_common.h"
#include "pulse.h"
#include "sim_dev.h"
#include <cmath>

namespace mbfir {

#define TRAIN_LSQ_KERNEL(name) name##_mag
#define TRAIN_MAG true
#include "blochtraingn_lsq.inc"
#include "blochtrainschedgn_lsq.inc"
#undef TRAIN_LSQ_KERNEL
#undef TRAIN_MAG

void train_run_lsq_mag_launch(hipStream_t st, long nblk, const double* ws, const double2* rep, const int* gidx, const double* rw,
                              const BlochPulseDev* pulses, const TrainPulseDev* trains, const SimBlock* blocks, const BlochCkDev* cks,
                              const long* lp, const double* m0, int demod, int ebcast, const double* we, const double* te, long PE,
                              const double* wf, const double* tf, long PO, double* ck, double* cw, double* gmx, double* gmy,
                              double* gmz, double* lpart) {
    hipLaunchKernelGGL(k_bloch_train_run_lsq_mag, dim3((unsigned)nblk), dim3(256), 0, st, ws, rep, gidx, rw, pulses, trains, blocks, cks,
                       lp, m0, demod, ebcast, we, te, PE, wf, tf, PO, ck, cw, gmx, gmy, gmz, lpart);
}
void train_sched_lsq_mag_launch(hipStream_t st, long nblk, const double* ws, const double* dws, const double2* rep, const int* gidx,
                                const double* rw, const BlochPulseDev* pulses, const TrainPulseDev* trains, const SimBlock* blocks,
                                const VjpPulseDev* vp, const BlochCkDev* cks, const long* lp, const double* m0, int demod, int ebcast,
                                const double* we, const double* te, long PE, const double* wf, const double* tf, long PO, double* ck,
                                double2* part, double* gmx, double* gmy, double* gmz, double* lpart) {
    hipLaunchKernelGGL(k_bloch_train_run_sched_lsq_mag, dim3((unsigned)nblk), dim3(256), 0, st, ws, dws, rep, gidx, rw, pulses, trains,
                       blocks, vp, cks, lp, m0, demod, ebcast, we, te, PE, wf, tf, PO, ck, part, gmx, gmy, gmz, lpart);
}

}  // namespace mbfir
