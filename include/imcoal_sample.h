/* imcoal_sample.h - drawing alignments from an HMM (pi, T, E): simulated replicates for the simulate -> prepare ->
 * estimate loop and for parametric bootstraps, written straight into device memory so that imc_obs_create_device
 * (imcoal_fwd.h) can build chunks from them without a symbol on the host.  NOT part of the forward boundary
 * (include/imcoal_fwd.h is), like imcoal_model.h.
 *
 * The output is defined by the sequential loop of csrc/sample_tiles.hpp and is exactly reproducible from (seed, tag):
 *   uniforms    Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (t & 0xffffffff, t >> 32, replicate, tag) for
 *               column t of a replicate; u_state from output words 0 and 1, u_sym from words 2 and 3, 53 bits each
 *   tables      per row, in fp64 on the host: running sum from left to right divided by its last value; every entry from
 *               the last strictly positive one onward is exactly 1.0; a draw takes the smallest j with u < cdf[j].  Rows
 *               need not be normalised.  A negative or non-finite entry, or a row whose total is not positive, is
 *               IMC_ERR_ARG; the message names the matrix and the row
 *   chain       x_0 from pi with u_state(0), x_t from row x_{t-1} of T with u_state(t), o_t from row x_t of E with u_sym(t)
 * Only the first emit_symbols columns of E (row stride S) are used, 1 <= emit_symbols <= S: the models here put 1.0 in the
 * missing-data column, so pairwise models are sampled with emit_symbols = 2.
 *
 * Arguments: pi [N], T [N][N], E [N][S] row-major host arrays; outputs laid out [replicate][column]: symbols of sym_bytes
 * (1 or 2) bytes each, and the hidden states as bytes unless states_out is NULL.  Limits, all IMC_ERR_ARG before any HIP
 * call: 1 <= N <= 256, 1 <= S <= 4096, sym_bytes == 1 requires emit_symbols <= 256, 1 <= L < 2^31,
 * 1 <= n_replicates <= 65536, no null pointers (states_out excepted).
 *
 * imc_sample_host   the sequential specification; needs no device.
 * imc_sample_device the same bytes from three kernel launches (csrc/kernels_sample.hpp: tile summaries as maps on the state
 *                   space, one scan, emission) into DEVICE memory.  Output pointers are checked like imc_obs_create_device's
 *                   d_sym (host memory is IMC_ERR_ARG, never a fault).  The work is enqueued under the library's mutex on
 *                   hip_stream (NULL: the default stream, as in imc_forward_batch_device); the call returns after
 *                   synchronising that stream.  No usable device: IMC_ERR_NODEVICE.  The stream is cut into tiles of
 *                   IMC_SAMPLE_TILE columns (environment, 1 .. 65536, read at every call; anything else is IMC_ERR_ARG);
 *                   no result depends on it.  A call whose stream has 2^31 tiles or more is IMC_ERR_ARG.
 * imc_last_sampling {path: 0 host / 1 device, tiles, tile length, columns} of this process's last successful call
 *                   (tiles and tile length are 0 for the host path). */
#ifndef IMCOAL_SAMPLE_H
#define IMCOAL_SAMPLE_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
int imc_sample_host(int N, int S, int emit_symbols, const double *pi, const double *T, const double *E, uint64_t seed,
                    uint32_t tag, int n_replicates, size_t L, void *sym_out, int sym_bytes, uint8_t *states_out);
int imc_sample_device(int N, int S, int emit_symbols, const double *pi, const double *T, const double *E, uint64_t seed,
                      uint32_t tag, int n_replicates, size_t L, void *d_sym_out, int sym_bytes, uint8_t *d_states_out,
                      void *hip_stream);
int imc_last_sampling(uint64_t *out4);
#ifdef __cplusplus
}
#endif
#endif /* IMCOAL_SAMPLE_H */
