// What the instrumented builds of the task queue report on stderr after a launch (host side; the counters and the CT_LOG macros
// are next to the device code that fills them, chol_queue.hpp):
//   -DALABI_CHOL_PROF  phase timers of the CHAIN and UPDATE tasks and of the diagonal factorisation (tools/run_chol_phases.sh)
//   -DALABI_CHOL_LOG   the CHAIN tasks' event log, printed when ALABI_CHOL_LOG_PRINT is set (tools/run_chol_log.sh)
// An ordinary build prints nothing.  Included by gp_cholesky.hip behind chol_queue.hpp.
#pragma once

namespace alabi {

static void chol_report_instrumentation(alabi_gp* gp, int nb, const CholSwitches& sw, hipStream_t s) {
    (void)gp; (void)nb; (void)sw; (void)s;
#ifdef ALABI_CHOL_PROF
    {
        long long h[24];
        (void)hipMemcpyAsync(h, gp->chol_ctl + ((2 + nb * nb + nb + 1) & ~1), sizeof(h), hipMemcpyDeviceToHost, s);
        (void)hipStreamSynchronize(s);
        for (int q = 8; q <= 16; q += 8)
            if (h[q + 4] > 0)
                fprintf(stderr, "[chol_tasks_kernel] per %s UPDATE (us): wait for deps %.2f, first fetch + C %.2f, loop %.2f (%.2f per block column), C store + publish %.2f (n=%lld, %.2f columns each)\n",
                        q == 8 ? "grouped" : "single-column", 0.01 * h[q] / h[q + 4], 0.01 * h[q + 1] / h[q + 4], 0.01 * h[q + 2] / h[q + 4],
                        0.01 * h[q + 2] / (h[q + 5] ? h[q + 5] : 1), 0.01 * h[q + 3] / h[q + 4], h[q + 4], (double)h[q + 5] / h[q + 4]);
        {
            long long pp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            (void)hipMemcpyFromSymbol(pp, HIP_SYMBOL(g_potrf_prof), sizeof(pp));
            if (pp[1] > 0) fprintf(stderr, "[chol_tasks_kernel] slab recurrence of the diagonal factorisation (wave 0): %.2f us per 16 pivots (n=%lld)\n", 0.01 * pp[0] / pp[1], pp[1]);
            if (pp[5] > 0) fprintf(stderr, "[chol_tasks_kernel] per factorisation (us): slabs 0-2 start -> barrier A %.2f each, A -> B %.2f each, last slab incl. its stores %.2f (n=%lld)\n",
                                   0.01 * pp[2] / (3 * pp[5]), 0.01 * pp[3] / (3 * pp[5]), 0.01 * pp[4] / pp[5], pp[5]);
            long long z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            (void)hipMemcpyToSymbol(HIP_SYMBOL(g_potrf_prof), z, sizeof(z));
        }
        if (h[6] > 0)
            fprintf(stderr, "[chol_tasks_kernel] per CHAIN (us): wait %.2f loads %.2f trsm %.2f store+publish %.2f mfma %.2f potrf %.2f store+publish %.2f (n=%lld)\n",
                    0.01 * h[7] / h[6], 0.01 * h[0] / h[6], 0.01 * h[1] / h[6], 0.01 * h[2] / h[6], 0.01 * h[3] / h[6], 0.01 * h[4] / h[6],
                    0.01 * h[5] / h[6], h[6]);
    }
#endif
#ifdef ALABI_CHOL_LOG
    if (sw.log_print) {
        static long long h[256][32];
        (void)hipStreamSynchronize(s);
        (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_chain_log), sizeof(h));
        const char* name[15] = {"drawn -> deps met", "deps met -> tiles in LDS", "tiles in LDS -> slab 0 seen", "slab 0 -> slab 1 seen", "slab 1 -> slab 2 seen",
                                "slab 2 -> slab 3 seen", "slab 3 seen -> solve + diag update done", "-> panel tile published", "-> factorisation starts",
                                "-> recurrence 0 done", "-> recurrence 1 done", "-> recurrence 2 done", "-> recurrence 3 done", "-> last inverse block out",
                                "-> tile stored, published"};
        const int k0 = nb / 4, k1 = nb - 2;
        fprintf(stderr, "[chain log] nb = %d, means over CHAIN(%d..%d), us:\n", nb, k0, k1);
        for (int i = 0; i < 15; ++i) {
            double sum = 0;
            for (int k = k0; k <= k1; ++k) sum += 0.01 * (double)(h[k][i + 1] - h[k][i]);
            fprintf(stderr, "  %-44s %7.2f\n", name[i], sum / (k1 - k0 + 1));
        }
        {
            double t[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = k0; k <= k1; ++k) {
                const long long r3 = h[k - 1][13];              // the producer's last recurrence done
                t[0] += 0.01 * (double)(h[k][3] - r3); t[1] += 0.01 * (double)(h[k][4] - r3); t[2] += 0.01 * (double)(h[k][5] - r3); t[3] += 0.01 * (double)(h[k][6] - r3);
                t[4] += 0.01 * (double)(h[k][7] - r3); t[5] += 0.01 * (double)(h[k][9] - r3); t[6] += 0.01 * (double)(h[k - 1][14] - r3); t[7] += 0.01 * (double)(h[k][2] - r3);
            }
            const double n_ = k1 - k0 + 1;
            fprintf(stderr, "  relative to the END of the previous CHAIN's last recurrence: tiles in LDS %+.2f; slab 0 / 1 / 2 / 3 in LDS %+.2f %+.2f %+.2f %+.2f; solve + diag update done %+.2f; "
                            "factorisation starts %+.2f (the previous CHAIN's last inverse block drained at %+.2f)\n", t[7] / n_, t[0] / n_, t[1] / n_, t[2] / n_, t[3] / n_, t[4] / n_, t[5] / n_, t[6] / n_);
        }
        for (int sl = 0; sl < 3; ++sl) {
            double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
            for (int k = k0; k <= k1; ++k) { a0 += 0.01 * (double)(h[k][16 + 4 * sl] - h[k][10 + sl]); a1 += 0.01 * (double)(h[k][17 + 4 * sl] - h[k][16 + 4 * sl]); a2 += 0.01 * (double)(h[k][18 + 4 * sl] - h[k][17 + 4 * sl]); a3 += 0.01 * (double)(h[k][19 + 4 * sl] - h[k][18 + 4 * sl]); }
            const double n_ = k1 - k0 + 1;
            fprintf(stderr, "  slab %d, storing wave 7: sees the recurrence done after %.2f, LDS reads %.2f, stores issued %.2f, drained %.2f\n", sl, a0 / n_, a1 / n_, a2 / n_, a3 / n_);
        }
        double per = 0, hop = 0;
        for (int k = k0; k <= k1; ++k) { per += 0.01 * (double)(h[k + 1][9] - h[k][9]); hop += 0.01 * (double)(h[k + 1][6] - h[k][14]); }
        fprintf(stderr, "  period (factorisation start to start) %.2f; last inverse block out -> seen by the next CHAIN %.2f\n", per / (k1 - k0 + 1), hop / (k1 - k0 + 1));
    }
#endif
}

}  // namespace alabi
