/*
 * mtscomp_hip.h -- C ABI of libmtscomp_hip.so: mtscomp's per-chunk codec on MI355X (gfx950).
 *
 * The reference (int-brain-lab/mtscomp, pure Python) has no FFI for this path: the hot path sits
 * behind Python methods that call numpy and the stdlib zlib module.  The entry points below are
 * what a ctypes binding of that path binds (INTEGRATION.md shows the stub).  Each one cites the
 * reference interface it replaces (file:line in /root/reference/mtscomp.py).
 *
 * Conventions: plain C types; the caller owns every buffer; return value 0 (MTS_OK) or a negative
 * MTS_E_* code (no exceptions cross the boundary); every call is re-entrant and thread-safe (calls on
 * one device are serialised inside the library); ctypes releases the GIL for the duration.
 * There is NO CPU fallback: without a usable gfx950 device every compute entry point returns
 * MTS_E_NODEV.
 *
 * `flags`: bit0 do_time_diff, bit1 do_spatial_diff, bit2 chunk_order=='F'   (reference config keys,
 * mtscomp.py:52-55), bit3 items are IEEE floats.  `level`: zlib level 1..9 or -1 (= 6), every one
 * byte-identical to zlib.compress(stream, level) of libz 1.2.11; the reference always compresses at
 * zlib's default (6) whatever `comp_level` says (mtscomp.py:394), so 6/-1 is the drop-in value.
 * Supported item types: integer dtypes of 1, 2, 4 or 8 bytes (two's complement wrap, like numpy) and,
 * with MTS_FLAG_FLOAT, float32 / float64 (np.diff / np.cumsum in the item type, bit for bit).
 */
#ifndef MTSCOMP_HIP_H
#define MTSCOMP_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define MTS_OK 0
#define MTS_E_ARG (-1)         /* bad argument */
#define MTS_E_NODEV (-2)       /* no usable gfx950 device / HIP runtime */
#define MTS_E_HIP (-3)         /* HIP runtime error (see mts_last_error) */
#define MTS_E_NOMEM (-4)       /* device or host allocation failed */
#define MTS_E_UNSUPPORTED (-5) /* valid request this build does not implement (e.g. the match-table tap at levels 1..3) */
#define MTS_E_INTERNAL (-6)    /* internal consistency check failed */
#define MTS_E_MISS (-7)        /* mts_cache_read_rows: a chunk given without bytes is not resident (any more) */

/* per-chunk status written by mts_decompress_chunks */
#define MTS_CHUNK_OK 0
#define MTS_CHUNK_CORRUPT (-1)    /* zlib.decompress would raise  -> IOError, mtscomp.py:618-621 */
#define MTS_CHUNK_BADSIZE (-2)    /* valid stream (check value included) of the wrong length -> AssertionError, mtscomp.py:628;
                                     a damaged stream of the wrong length is MTS_CHUNK_CORRUPT, as zlib reports it first */

#define MTS_FLAG_TIME_DIFF 1
#define MTS_FLAG_SPATIAL_DIFF 2
#define MTS_FLAG_ORDER_F 4
#define MTS_FLAG_FLOAT 8          /* items are IEEE floats (itemsize 4 or 8): np.diff / np.cumsum in that type, bit for bit */
#define MTS_FLAG_UNSIGNED 16      /* integer items are unsigned (mts_window_stats, mts_decimate, mts_project, mts_detect, mts_waveforms, mts_waveform_features, mts_localize, mts_correlate, mts_match_templates, mts_welch, mts_gram and their device variants only; the codec does not care) */
#define MTS_DECIMATE_MAX_TAPS 8192
#define MTS_PROJECT_MAX_COLS 1024
#define MTS_PROJECT_MAX_OUT  1024
#define MTS_WELCH_MAX_NPERSEG 16384
#define MTS_WELCH_BLOCK_SEGMENTS 32   /* mts_welch: segments per block (B), summed in order on the device */
#define MTS_WELCH_GROUP_ROWS (1l << 20) /* a group is the smallest multiple G of B segments with G * step >= this many rows */
#define MTS_GRAM_GROUP_ROWS (1l << 20)  /* mts_gram: rows per group of a window (aligned to the window's start; the last may be short) */
#define MTS_GRAM_SLAB_ROWS 4096         /* mts_gram: rows per slab of a group (aligned to the group's start; the last may be short) */
#define MTS_GRAM_MAX_COLS 16384
#define MTS_DETECT_MAX_EXCLUDE 255      /* mts_detect: rows either side in which a larger sample suppresses an event */
#define MTS_DETECT_MAX_SPREAD 32        /* ... and column positions either side */
#define MTS_WAVEFORMS_MAX_ROWS 4096     /* mts_waveforms: rows of a snippet (before + after) */
#define MTS_WAVEFORMS_MAX_WIDTH 1024    /* ... and its column positions */
#define MTS_MEAN_MAX_LABELS 4096       /* mts_mean_waveforms: labels of a call */
#define MTS_MEAN_MAX_ENTRIES (1L << 27) /* ... and n_labels * T * width, the entries of its sums */
#define MTS_FEATURES_MAX_COMPONENTS 32  /* mts_waveform_features: rows of its basis (the components) */
#define MTS_FEATURES_MAX_BASIS 8192     /* ... and n_comp * T, the entries of the basis: 32 KiB of LDS */
#define MTS_LOCALIZE_MAX_DIMS 4         /* mts_localize: coordinates of a channel position */
#define MTS_LOCALIZE_PTP 0              /* ... its amplitude modes: maximum - minimum of a column */
#define MTS_LOCALIZE_NEG 1              /* ... -minimum (detect's sign 'neg') */
#define MTS_LOCALIZE_POS 2              /* ... maximum ('pos') */
#define MTS_LOCALIZE_ABS 3              /* ... maximum of the absolute values ('abs') */
#define MTS_DETECT_MAX_REF_COLS 1024    /* columns of a median reference: a row's order keys are sorted in 4 KiB of LDS by one wave */
#define MTS_CORRELATE_MAX_T 256         /* mts_correlate: rows of a template (its taus) */
#define MTS_CORRELATE_MAX_OUT 1024      /* ... the templates of a call */
#define MTS_CORRELATE_MAX_COLS 1024     /* ... and the columns of one */
#define MTS_TMATCH_MAX_EXCLUDE 255      /* mts_match_templates: rows either side in which a larger score suppresses an event */

int mts_version(void);
int mts_device_count(void);                 /* number of gfx950 devices visible; 0 if none */
const char *mts_strerror(int code);
const char *mts_last_error(void);           /* thread-local detail of the last failure */

/* zlib's compressBound(): capacity to reserve per chunk slot */
long mts_compress_bound(long raw_len);

/*
 * diff_along_axis(axis=0/1) + ndarray.tobytes(order)            mtscomp.py:143-159, :381-382, :394
 * raw: C-order (n_samples, n_channels).  stream_out: n_samples*n_channels*itemsize bytes.
 */
int mts_delta_transpose(int device, const void *raw, long n_samples, int n_channels, int itemsize,
                        int flags, void *stream_out);

/*
 * reshape(order) + cumsum_along_axis(axis=1/0) + ascontiguousarray   mtscomp.py:622-635, :162-169
 * stream: the inflated bytes of one chunk.  out: C-order (n_samples, n_channels).
 */
int mts_cumsum_transpose(int device, const void *stream, long n_samples, int n_channels,
                         int itemsize, int flags, void *out);

/*
 * One batch of Writer._compress_chunk calls -- replaces `pool.map(self._compress_chunk, range(...))`
 * (mtscomp.py:375-397, :399-423).
 *   raw            C-order (rows, n_channels) array holding rows [chunk_bounds[0], chunk_bounds[n_chunks])
 *                  -- i.e. `raw` points at row chunk_bounds[0]
 *   chunk_bounds   n_chunks+1 row indices; chunk i = rows [b[i], b[i+1])        (mtscomp.py:324-339)
 *   out            caller buffer; chunk i's zlib stream is written at out + out_slot_offsets[i], which
 *                  must have room for mts_compress_bound(len_i) bytes
 *   out_sizes      n_chunks compressed lengths (what `len(chunkdc)` is in mtscomp.py:478)
 * Output bytes are identical to zlib.compress() of libz 1.2.11 at `level`.
 */
int mts_compress_chunks(int device, const void *raw, int n_channels, int itemsize,
                        const long *chunk_bounds, int n_chunks, int flags, int level,
                        unsigned char *out, const long *out_slot_offsets, long *out_sizes);

/*
 * One batch of Reader.read_chunk calls -- replaces `pool.map(self._decompress_chunk, ids)`
 * (mtscomp.py:602-643, :645-650).  Chunks need not be adjacent in the file.
 *   cdata          base of the compressed bytes the caller read (os.pread, mtscomp.py:609)
 *   c_offsets      n_chunks byte offsets into cdata;  c_lengths: n_chunks byte lengths
 *   n_rows         n_chunks row counts (chunk_bounds[i+1] - chunk_bounds[i])
 *   out            caller buffer;  chunk i's C-order (n_rows[i], n_channels) array goes to
 *                  out + out_offsets[i] (bytes)
 *   chunk_status   MTS_CHUNK_* per chunk; a corrupt chunk does not stop the others (mtscomp.py:621)
 * Accepts any valid RFC 1950/1951 stream (stored/fixed/dynamic blocks, any encoder); verifies adler32;
 * ignores trailing bytes after the stream like zlib.decompress does.
 */
int mts_decompress_chunks(int device, const unsigned char *cdata, const long *c_offsets,
                          const long *c_lengths, const long *n_rows, int n_chunks, int n_channels,
                          int itemsize, int flags, void *out, const long *out_offsets,
                          int *chunk_status);

/*
 * Reader random access (Reader.__getitem__, mtscomp.py:798-856, with read_chunk's lru_cache of decoded chunks,
 * mtscomp.py:582-588, :602) -- the cache lives in HBM: decoded chunks stay on the device and a slice costs one
 * device-to-host copy of exactly the requested rows.
 *   mts_cache_create    capacity in bytes of decoded chunks (least recently used chunks are dropped beyond it)
 *   mts_cache_query     present[i] = 0 if the decoded chunk with key chunk_keys[i] is not resident, else the number of channels
 *                       the entry holds (n_channels, or the leading channels of mts_cache_read_slices_leading)
 *   mts_cache_read_slices  (below) any number of row/column rectangles per call, gathered on the device
 *   mts_cache_read_rows the chunks of one slice, in file order: resident ones may come with c_lengths[i] = 0, the others
 *                       with their compressed bytes (cdata + c_offsets[i], c_lengths[i]) and are decoded in one batch and
 *                       kept.  Rows [row_begin, row_end) of the concatenation of the n_chunks chunks are written to `out`
 *                       (C order).  chunk_status as in mts_decompress_chunks (rows of a failed chunk are not written).
 *                       MTS_E_MISS: a chunk given without bytes is not resident -- call again with its bytes.
 * Keys are the caller's (the Reader uses the chunk index; one cache per open file).
 */
int mts_cache_create(int device, long capacity_bytes, long *cache_id);
int mts_cache_destroy(long cache_id);
int mts_cache_query(long cache_id, const long *chunk_keys, int n, int *present);
int mts_cache_read_rows(long cache_id, int n_chunks, const long *chunk_keys, const unsigned char *cdata,
                        const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels,
                        int itemsize, int flags, long row_begin, long row_end, void *out,
                        int *chunk_status);
/* Several rectangular pieces in one call -- Reader[rows, columns] (mtscomp.py:835-842, where the reference decodes whole
 * chunks and drops rows and columns on the host) and many slices per launch.  The chunks are the union of what the requests
 * touch (file order, every key once; residency and bytes as in mts_cache_read_rows).  Request k is six longs,
 *   row_begin, row_end, row_step (>= 1), col_begin, col_end, col_step (>= 1),
 * rows counted in the concatenation of the listed chunks; its ceil((row_end - row_begin) / row_step) x
 * ceil((col_end - col_begin) / col_step) items are gathered ON THE DEVICE and written C-contiguous at out + out_offsets[k]
 * (bytes); the out_bytes of `out` cross the bus in one copy and nothing else does.  Rows of a failed chunk are not written. */
int mts_cache_read_slices(long cache_id, int n_chunks, const long *chunk_keys, const unsigned char *cdata,
                          const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels,
                          int itemsize, int flags, int n_requests, const long *requests, void *out,
                          const long *out_offsets, long out_bytes, int *chunk_status);
/* The same for requests that only touch the first n_leading channels of channel-major integer chunks (chunk_order 'F', the
 * reference's default: the stream of a chunk is channel after channel, so the leading channels are a PREFIX of it): a chunk that
 * is not resident is inflated only until that prefix is complete -- whole deflate blocks, no adler32 check, which needs the
 * whole stream -- and kept as a (rows, n_leading) entry; c_lengths[i] may then be a prefix of the chunk's compressed bytes
 * (about n_leading / n_channels of them plus a margin).  MTS_E_MISS: the bytes given do not reach the prefix, or a resident entry
 * holds fewer channels than asked for -- call again with more bytes.  Column ranges of the requests must end at or before
 * n_leading.  n_leading == n_channels is mts_cache_read_slices.  (The reference decodes whole chunks and drops columns on the
 * host, mtscomp.py:835-842.)
 * How many bytes are enough: those up to and including the byte that holds the last bit of the deflate block that completes the
 * prefix, no slack behind it (tests/test_gpu_prefix_reads.py, PREFIX_SLACK_BYTES = 0) -- also when that block is the chunk's last
 * one: the check value behind it is never looked at, so a chunk cut inside its 4-byte trailer is as good as a whole one.  Any
 * shorter prefix of an intact chunk, and a stream the block-parallel decoder cannot follow up to there (fixed or stored blocks the
 * scan does not announce, beyond a short one), is MTS_E_MISS, never MTS_CHUNK_CORRUPT / MTS_CHUNK_BADSIZE and never wrong bytes. */
int mts_cache_read_slices_leading(long cache_id, int n_chunks, const long *chunk_keys, const unsigned char *cdata,
                                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels,
                                  int itemsize, int flags, int n_leading, int n_requests, const long *requests,
                                  void *out, const long *out_offsets, long out_bytes, int *chunk_status);

/*
 * Per-window, per-channel statistics of decoded chunks (an extension: the reference has no such call; its users reduce
 * Reader[...] with numpy).  Only the results cross the bus.
 *   windows        [row_begin + w * window_rows, min(row_begin + (w + 1) * window_rows, row_end)) for
 *                  w < ceil((row_end - row_begin) / window_rows), in absolute file rows
 *   chunks         chunk i holds file rows [chunk_row0[i], chunk_row0[i] + n_rows[i]); ascending, not overlapping, not
 *                  necessarily adjacent (a lane of a multi-device caller gets every G-th chunk); every chunk must hold a row of
 *                  [row_begin, row_end).  A call reduces the rows of its chunks only.
 *   cols           n_cols >= 1 channel indices, any order, repeats allowed
 *   flags          as everywhere; MTS_FLAG_FLOAT for float items, MTS_FLAG_UNSIGNED for unsigned integers (signed otherwise)
 *   outputs        (n_windows, n_cols) C order:
 *                    out_min / out_max  the item type; floats propagate NaN like np.min / np.max
 *                    out_sum            int64 (x.astype(int64).sum(0), two's-complement wrap) for integers, double for floats
 *                    out_sumsq          uint64 -- the EXACT sum of squares -- for 1- and 2-byte integers (windows of up to 2^31 rows);
 *                                       double accumulation for 4/8-byte integers and floats.  A caller combining several calls
 *                                       adds the uint64 sums and converts once.
 *                    out_count          (n_windows) rows of the window held by the chunks that decoded
 *                  A window with no row in these chunks gets the identities: type max / +inf, type min / -inf, 0, 0, count 0.
 *                  Nothing is atomic: the double sums are the same from run to run.
 *   chunk_status   MTS_CHUNK_* per chunk as in mts_decompress_chunks; the rows of a failed chunk count nowhere
 * mts_window_stats: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated (whole chunks, adler32 checked) and
 * reduced piece by piece in a transient workspace, the compressed bytes of the next piece crossing the bus beside the kernels; they
 * are NOT inserted into the cache.  Outputs are host memory.
 * mts_dev_window_stats: device d_cdata and d_* outputs on `device`, count and chunk_status on the host; no cache.
 * MTS_E_ARG before anything is launched: window_rows < 1, n_cols < 1, a column outside [0, n_channels), chunks out of order or
 * outside the range, an empty chunk, or a window of more than 2^31 rows on the exact (1/2-byte integer) path.
 */
int mts_window_stats(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0,
                     const unsigned char *cdata, const long *c_offsets, const long *c_lengths, const long *n_rows,
                     int n_channels, int itemsize, int flags, long row_begin, long row_end, long window_rows, int n_cols,
                     const int *cols, void *out_min, void *out_max, void *out_sum, void *out_sumsq, long *out_count,
                     int *chunk_status);

/*
 * FIR low-pass and decimation of decoded chunks (an extension: the reference has no such call; its users filter Reader[...] on
 * the host, e.g. with scipy.signal.decimate).  Only the outputs cross the bus.
 *   outputs        y[k, c] = sum_{j=0..n_taps-1} taps[j] * x[first_row + k * q - j, cols[c]] for k < n_out, in absolute file rows;
 *                  x is 0 outside [valid_begin, valid_end).  (n_out, n_cols) C order, float (out_itemsize 4) or double (8).
 *                  Items and taps are converted to that type with round-to-nearest; every output is acc = 0, then
 *                  acc = acc + taps[j] * x for j = 0, 1, .. in that type, product and sum each rounded (no fused multiply-add):
 *                  the same bits whatever the call, its pieces or the device.  Zero taps are not skipped (inf * 0 is NaN).
 *   q, taps        q >= 1; 1 <= n_taps <= MTS_DECIMATE_MAX_TAPS finite doubles on the host, not normalised
 *   chunks         chunk i holds file rows [chunk_row0[i], chunk_row0[i] + n_rows[i]); adjacent and ascending; together they
 *                  must cover the rows the outputs read: [first_row - n_taps + 1, first_row + (n_out - 1) * q] ∩ [valid_begin,
 *                  valid_end)
 *   cols           n_cols >= 1 channel indices, any order, repeats allowed
 *   flags          as everywhere; MTS_FLAG_FLOAT for float items, MTS_FLAG_UNSIGNED for unsigned integers (signed otherwise)
 *   chunk_status   MTS_CHUNK_* per chunk as in mts_decompress_chunks; the outputs that read a failed chunk are undefined
 * mts_decimate: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated (whole chunks, adler32 checked) piece
 * by piece (MTS_PIPE_BYTES) in a transient workspace, the compressed bytes of the next piece crossing the bus beside the kernels;
 * a chunk below a piece boundary that outputs of both pieces read is inflated in both.  They are NOT inserted into the cache.
 * `out` is host memory.
 * mts_dev_decimate: device d_cdata and d_out on `device`, chunk_status on the host; no cache.
 * MTS_E_ARG before anything is launched: q < 1, n_taps outside [1, MTS_DECIMATE_MAX_TAPS], a tap that is not finite, out_itemsize
 * not 4 or 8, n_cols < 1, a column outside [0, n_channels), chunks not adjacent or not covering the rows read, an empty chunk.
 */
int mts_decimate(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0,
                 const unsigned char *cdata, const long *c_offsets, const long *c_lengths, const long *n_rows,
                 int n_channels, int itemsize, int flags, long valid_begin, long valid_end, long first_row, long n_out,
                 int q, int n_taps, const double *taps, int out_itemsize, int n_cols, const int *cols, void *out,
                 int *chunk_status);

/*
 * Channel-mixing matrix products of decoded chunks (an extension: the reference has no such call; its users form Reader[...] @ W on
 * the host).  Whitening, projection onto principal components, re-referencing, selecting and scaling channels are all this one
 * row-by-row product.  Only the outputs cross the bus.
 *   outputs        y[t, k] = sum_{j < n_cols} (x[t, cols[j]] - offset[j]) * weights[j, k] for row_begin <= t < row_end, k < n_out, in
 *                  absolute file rows.  (row_end - row_begin, n_out) C order, F = float (out_itemsize 4) or double (8).
 *   the chain      Items, offsets and weights are each rounded once to F (items as mts_decimate converts them, unsigned by
 *                  MTS_FLAG_UNSIGNED); d[t, j] = F(x[t, cols[j]]) - F(offset[j]) is one IEEE subtraction in F; offset NULL means zeros.
 *                  With n4 = n_cols rounded up to a multiple of 4, positions j >= n_cols enter as d = 0, w = 0.  y[t, k] is the chain
 *                  of 4-column matrix steps over j = 0, 4, 8, .. < n4, in that order, from +0; each step is one
 *                  v_mfma_f32_16x16x4_f32 (v_mfma_f64_16x16x4_f64) with d[t, j .. j + 3] as A and w[j .. j + 3, k] as B.  Zero
 *                  weights are not skipped (inf * 0 is NaN).  y[t, k] depends on row t, cols, offset and column k of weights alone:
 *                  not on the tile it lands in, the other output columns, the chunks, pieces, calls, lanes, cache residency or device.
 *   float          a float32 step is bit for bit the k-ordered chain acc = fmaf(d_j, w_jk, acc), so y[t, k] is that chain over
 *                  j = 0 .. n4 - 1 from +0: a definition, not a tolerance.  float32 subnormals are kept, as operands and as results
 *                  (the kernels are built with hipcc's default float mode).
 *   double         held to a bound, as mts_gram is: with u = 2^-53, |y - sum_j (x_j - o_j) w_jk| <= gamma_{n4+4} * sum_j (|x_j| + |o_j|)
 *                  |w_jk| + n4 * 2^-1074 (item / offset conversion, subtraction, weight, and at most n4 roundings of the chain; the
 *                  absolute term is the gradual underflow).  The same bound with u = 2^-24 and 2^-149 holds for float.
 *   limits         1 <= n_cols <= MTS_PROJECT_MAX_COLS channel indices, any order, repeats allowed; 1 <= n_out <= MTS_PROJECT_MAX_OUT;
 *                  weights (n_cols, n_out) C order and offset (n_cols or NULL) finite doubles on the host
 *   chunks         as mts_decimate: adjacent, ascending, covering [row_begin, row_end).  row_begin == row_end is MTS_OK with nothing
 *                  written.
 *   chunk_status   MTS_CHUNK_* per chunk as in mts_decompress_chunks; the outputs of a failed chunk's rows are undefined
 * mts_project: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated (whole chunks, adler32 checked) piece
 * by piece (MTS_PIPE_BYTES) in a transient workspace, the compressed bytes of the next piece crossing the bus beside the kernels; a
 * piece owns the rows of its chunks, so no chunk is inflated twice.  They are NOT inserted into the cache.  `out` is host memory.
 * mts_dev_project: device d_cdata and d_out on `device`, chunk_status on the host; no cache.
 * MTS_E_ARG with a message before anything is allocated or launched: n_cols or n_out outside their limits, a weight or an offset
 * that is not finite, out_itemsize not 4 or 8, a column outside [0, n_channels), row_begin < 0 or row_end < row_begin, no output
 * buffer, chunks not adjacent or not covering the rows, an empty chunk.
 */
int mts_project(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                long row_end, int n_cols, const int *cols, const double *offset /* n_cols or NULL */, int n_out,
                const double *weights /* (n_cols, n_out) C order */, int out_itemsize, void *out /* (row_end - row_begin, n_out) C order */,
                int *chunk_status);

/*
 * Threshold-crossing peak detection on filtered rows (an extension: the reference has no such call; its users filter Reader[...],
 * subtract a per-sample median and look for peaks on the host).  Only the events cross the bus.  Everything is float32 and a
 * definition, not a tolerance:
 *   filter         y[t, j] = sum_{k=0..n_taps-1} taps[k] * x[t + half - k, cols[j]], half = (n_taps - 1) / 2, x = 0 outside
 *                  [valid_begin, valid_end): the arithmetic of mts_decimate with q = 1 and out_itemsize 4, bit for bit
 *   reference      0: z = y.  1: z = y - m[t] (one rounding), m[t] the median of y[t, 0 .. n_cols) with repeated columns counted:
 *                  the values in np.sort's order, NaN last; the middle one for an odd n_cols, 0.5f * (a + b) of the two middle ones
 *                  (the sum rounded to float) for an even one; NaN when the row holds a NaN
 *   sign           0: v = -z, 1: v = z, 2: v = |z|
 *   event          (t, j) with row_begin <= t < row_end, v[t, j] > threshold[j] and no neighbour that beats it.  Neighbours:
 *                  (t', j') != (t, j) with |t' - t| <= exclude_rows, |j' - j| <= exclude_cols (positions in cols), valid_begin <= t'
 *                  < valid_end, 0 <= j' < n_cols -- inside or outside [row_begin, row_end).  It beats (t, j) when v' > v, or v' == v
 *                  and (t', j') precedes (t, j) in (t, j) order.  A NaN beats nothing and is no event; a plateau gives one event, at
 *                  its first row and lowest position.  Calls on [a, b) and [b, c) together give the events of [a, c).
 *   threshold      n_cols finite floats > 0 on the host
 *   outputs        the events in ascending (t, j) order: out_row[i] = t (file row), out_pos[i] = j, out_amp[i] = z[t, j].
 *                  *n_events: the events found, which may exceed max_events; then the first max_events of them are written and the
 *                  call still answers MTS_OK (call again with room for *n_events).  max_events 0: a count, the outputs may be null.
 *                  The same bytes whatever the call, its pieces, its slabs, the cache or the device.
 *   limits         1 <= n_taps <= MTS_DECIMATE_MAX_TAPS finite doubles; exclude_rows <= MTS_DETECT_MAX_EXCLUDE; exclude_cols <=
 *                  MTS_DETECT_MAX_SPREAD (a true peak visits (2 exclude_rows + 1) * (2 exclude_cols + 1) samples: the limits keep that
 *                  near 33000 loads); with a reference n_cols <= MTS_DETECT_MAX_REF_COLS
 *   chunks         as mts_decimate: adjacent, ascending, covering [row_begin - exclude_rows + half - n_taps + 1, row_end + exclude_rows +
 *                  half) within [valid_begin, valid_end); valid_begin <= row_begin <= row_end <= valid_end
 *   chunk_status   MTS_CHUNK_* per chunk; the events near a failed chunk are undefined
 * mts_detect: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated piece by piece (MTS_PIPE_BYTES) in a
 * transient workspace and NOT inserted; a piece owns the rows of its chunks and a chunk in the halo of two pieces is inflated in
 * both.  Within a piece the rows go through the float workspace in slabs of at most 256 MiB.  The outputs are host memory.
 * mts_dev_detect: device d_cdata and d_* outputs on `device`; threshold, n_events and chunk_status on the host; no cache.
 * MTS_E_ARG before anything is launched: any argument outside the ranges above, a threshold that is not a finite positive number,
 * a tap that is not finite, max_events < 0 or no output buffer for it, chunks not adjacent or not covering the rows read.
 */
int mts_detect(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
               const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
               long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols,
               const float *threshold, int sign, int reference, int exclude_rows, int exclude_cols, long max_events, long *out_row,
               int *out_pos, float *out_amp, long *n_events, int *chunk_status);

/*
 * Snippets around events and their extrema (an extension: the reference has no such call; its users pull Reader[...] across the bus,
 * filter it and slice on the host).  Only the snippets and four numbers per event cross the bus.  Everything is float32 and a
 * definition, not a tolerance:
 *   z              exactly mts_detect's z: the filter y[t, j] = sum_k taps[k] * x[t + half - k, cols[j]] (mts_decimate with q = 1 and
 *                  out_itemsize 4, bit for bit; x = 0 outside [valid_begin, valid_end)), and with reference 1 the float32 median over
 *                  all n_cols columns of row t subtracted (np.sort's order, NaN last, 0.5f * (a + b) for an even n_cols)
 *   snippet        event e at file row ev_row[e] with first column position ev_col0[e]: wave[e, tau, w] = z[ev_row[e] - before + tau,
 *                  ev_col0[e] + w] for 0 <= tau < T = before + after, 0 <= w < width
 *   fill           an entry whose row lies outside [valid_begin, valid_end) or whose column position lies outside [0, n_cols) is the
 *                  quiet NaN 0x7fc00000; an entry whose z is a NaN is stored as the same bits (the sign and payload that float
 *                  arithmetic gives a NaN differ from one processor to the next and are not part of the definition)
 *   extrema        out_min / out_argmin / out_max / out_argmax per event, over the entries that are not NaN (fill entries and NaN data
 *                  alike are ignored): arg* is the flat index tau * width + w of the first such entry in (tau, w) order; -0 and +0
 *                  compare equal, so the first wins and its own bits are returned; an event without such an entry gives NaN and -1
 *   events         n_events file rows on the host, ascending (repeats allowed), each in [valid_begin, valid_end); ev_col0 any int
 *   outputs        out_wave (n_events, T, width) C order, or null: the extrema alone, the same bytes as with it.  The same bytes
 *                  whatever the call, its pieces, its slabs, the gap setting, the cache or the device.
 *   limits         1 <= T <= MTS_WAVEFORMS_MAX_ROWS, before and after >= 0; 1 <= width <= MTS_WAVEFORMS_MAX_WIDTH; 0 <= n_events <=
 *                  2^40; taps and columns as mts_detect; with a reference n_cols <= MTS_DETECT_MAX_REF_COLS
 *   chunks         as mts_decimate: adjacent, ascending, covering [ev_row[0] - before + half - n_taps + 1, ev_row[n_events - 1] + after
 *                  + half) within [valid_begin, valid_end)
 *   chunk_status   MTS_CHUNK_* per chunk; the snippets near a failed chunk are undefined
 * mts_waveforms: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated piece by piece (MTS_PIPE_BYTES) in a
 * transient workspace and NOT inserted; a piece owns the events whose rows lie in its chunks.  Within a piece the events go through
 * the float workspace in slabs of at most 256 MiB (MTS_WAVEFORMS_SLAB_BYTES) that also end where the next event starts more than
 * MTS_WAVEFORMS_GAP_ROWS rows (4096; negative: never) past the rows filtered so far.  The outputs are host memory.
 * mts_dev_waveforms: device d_cdata and d_* outputs on `device`; ev_row, ev_col0 and chunk_status on the host; no cache.
 * MTS_E_ARG with a message before anything is allocated or launched: ev_row not ascending or a row outside [valid_begin, valid_end),
 * any argument outside the limits above, no extrema buffers, a tap that is not finite, chunks not adjacent or not covering the rows
 * read.  n_events == 0 is MTS_OK without a launch.
 */
int mts_waveforms(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                  long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                  const long *ev_row, const int *ev_col0, int before, int after, int width,
                  float *out_wave /* (n_events, T, width) C order or null */, float *out_min, int *out_argmin, float *out_max, int *out_argmax,
                  int *chunk_status);

/*
 * Per-label sums of the snippets of mts_waveforms, in fixed point (an extension: the reference has no such call; its users average the
 * snippets on the host).  What crosses the bus is n_labels * T * width sums and counts, not n_events * T * width floats.  A
 * definition, not a tolerance:
 *   z, T, entry    exactly mts_waveforms': z is mts_detect's z; the entry (e, tau, w), 0 <= tau < T = before + after, 0 <= w < width,
 *                  has the row r = ev_row[e] - before + tau and the column position c = ev_col0[e] + w
 *   clipping       an entry whose r lies outside [valid_begin, valid_end) or whose c lies outside [0, n_cols) contributes nothing and
 *                  is counted nowhere
 *   sum            every other entry takes d = (double)z[r, c] * (1 / resolution); resolution is a power of two in [2^-60, 2^60], so the
 *                  product is exact.  If z is a NaN or |d| >= 2^42 (+-inf included): out_skipped[ev_label[e]] += 1.  Otherwise
 *                  out_sum[ev_label[e], tau, w] += (int64)rint(d) and out_count[ev_label[e], tau, w] += 1; rint rounds to nearest,
 *                  ties to even
 *   events         as mts_waveforms: n_events file rows on the host, ascending (repeats allowed), each in [valid_begin, valid_end);
 *                  ev_col0 any int; 0 <= ev_label[e] < n_labels; at most 2^21 events of one label in a call, so that |sum| < 2^63
 *   outputs        out_sum (n_labels, T, width) int64, out_count (n_labels, T, width) int32, out_skipped (n_labels) int64, C order:
 *                  written whole by the call, zero where nothing was added.  Integer addition is associative: the same bytes whatever
 *                  the call, its pieces, its slabs, the gap setting, the split of a label's events into parts
 *                  (MTS_MEAN_PART_EVENTS), the cache or the device -- and the sums of several calls over a split event list add up
 *                  to the sums of one
 *   limits         T and width as mts_waveforms; 1 <= n_labels <= MTS_MEAN_MAX_LABELS; n_labels * T * width <= MTS_MEAN_MAX_ENTRIES;
 *                  taps and columns as mts_detect; with a reference n_cols <= MTS_DETECT_MAX_REF_COLS
 *   chunks, chunk_status   as mts_waveforms; the sums of labels with events near a failed chunk are undefined
 * mts_mean_waveforms: host cdata; cache_id 0 or a decoded-chunk cache, read in place and never inserted into, as mts_waveforms; the
 * same pieces (MTS_PIPE_BYTES) and slabs (MTS_WAVEFORMS_SLAB_BYTES, MTS_WAVEFORMS_GAP_ROWS).  The outputs are host memory.
 * mts_dev_mean_waveforms: device d_cdata and d_* outputs on `device`; ev_row, ev_col0, ev_label and chunk_status on the host; no cache.
 * MTS_E_ARG with a message before anything is allocated or launched: what mts_waveforms refuses, a label outside [0, n_labels), a label
 * with more than 2^21 events, a resolution that is not a power of two in range, any argument outside the limits above, no output
 * buffers.  n_events == 0 writes zeros and launches no gather.
 */
int mts_mean_waveforms(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                       const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                       long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                       const long *ev_row, const int *ev_col0, const int *ev_label, int n_labels, int before, int after, int width,
                       double resolution, long long *out_sum /* (n_labels, T, width) */, int *out_count /* (n_labels, T, width) */,
                       long *out_skipped /* (n_labels) */, int *chunk_status);

/*
 * The snippets of mts_waveforms projected on a small temporal basis: the "PC features" that clustering reads (an extension: the reference
 * has no such call; its users pull the snippets across the bus and run an einsum on the host).  What crosses the bus is n_events *
 * n_comp * width floats, not n_events * T * width.  Everything is float32 and a definition, not a tolerance:
 *   z, events, snippet, fill   exactly mts_waveforms': s[e, tau, w] is the entry that mts_waveforms returns, the quiet NaN 0x7fc00000
 *                  where its row lies outside [valid_begin, valid_end) or its column position outside [0, n_cols)
 *   basis          (n_comp, T) float32 in C order on the host, T = before + after; every entry finite
 *   features       out_feat[e, p, w] is the chain acc = +0; for tau = 0 .. T - 1: acc = fmaf(s[e, tau, w], basis[p, tau], acc), bit for
 *                  bit; a NaN result is stored as 0x7fc00000.  Zero basis entries are not skipped (inf * 0 is NaN), so one fill or NaN
 *                  entry in the column (e, ., w) makes out_feat[e, :, w] NaN.  From +0 the chain never ends at -0
 *   outputs        out_feat (n_events, n_comp, width) C order.  One chain is one thread's from +0 to its store: the same bytes
 *                  whatever the call, its pieces, its slabs, the gap setting, the cache or the device, and the bytes of the chain
 *                  applied on the host to mts_waveforms' own snippets
 *   limits         T, width, n_events, taps, columns and the reference's columns as mts_waveforms; 1 <= n_comp <=
 *                  MTS_FEATURES_MAX_COMPONENTS; n_comp * T <= MTS_FEATURES_MAX_BASIS
 *   chunks, chunk_status   as mts_waveforms; the features near a failed chunk are undefined
 * mts_waveform_features: host cdata; cache_id 0 or a decoded-chunk cache, read in place and never inserted into, as mts_waveforms; the
 * same pieces (MTS_PIPE_BYTES) and slabs (MTS_WAVEFORMS_SLAB_BYTES, MTS_WAVEFORMS_GAP_ROWS).  The output is host memory.
 * mts_dev_waveform_features: device d_cdata and d_feat on `device`; ev_row, ev_col0, basis and chunk_status on the host; no cache.
 * MTS_E_ARG with a message before anything is allocated or launched: what mts_waveforms refuses, n_comp or n_comp * T outside the
 * limits, no basis, no output buffer, a basis entry that is not finite.  n_events == 0 is MTS_OK without a launch.
 */
int mts_waveform_features(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                          const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                          long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                          const long *ev_row, const int *ev_col0, int before, int after, int width, int n_comp,
                          const float *basis /* (n_comp, T) C order */, float *out_feat /* (n_events, n_comp, width) C order */, int *chunk_status);

/*
 * Where on the probe a spike happened, and its amplitude on every channel of the snippet (an extension: the reference has no such call;
 * its users pull the snippets across the bus and run nanmax - nanmin and a weighted mean on the host).  What crosses the bus is
 * n_events * (width + n_dims + 2) numbers, not n_events * T * width.  Everything is float32 and a definition, not a tolerance:
 *   z, events, snippet, fill   exactly mts_waveforms': s[e, tau, w] is the entry that mts_waveforms returns, the quiet NaN 0x7fc00000
 *                  where its row lies outside [valid_begin, valid_end) or its column position outside [0, n_cols), and for a NaN of
 *                  the data
 *   extrema        of the column (e, ., w), over the entries that are not NaN: lo the first minimum, hi the first maximum, each with
 *                  its own bits (-0 == +0: the first wins, as mts_waveforms' extrema).  A column without such an entry has none
 *   amplitude      a[e, w] by mode: MTS_LOCALIZE_PTP hi - lo (one subtraction), MTS_LOCALIZE_NEG -lo (exact: +0 gives -0),
 *                  MTS_LOCALIZE_POS hi, MTS_LOCALIZE_ABS the first maximum of fabsf(entry); 0x7fc00000 for a column without extrema
 *                  and for a NaN result.  NaN entries are skipped (mts_waveforms' rule, not mts_waveform_features'): an event near
 *                  the recording's ends keeps the amplitudes of the rows it has
 *   weight         g[e, w] = a[e, w] if a[e, w] > 0, else +0 (NaN, negative and zero amplitudes: +0; +inf stays)
 *   sums           one chain per event over w = 0 .. width - 1 in ascending order, c = ev_col0[e] + w, a w with c outside [0, n_cols)
 *                  left out: out_weight[e] = (.. + g[e, w]), one addition a step, and out_moment[e, d] = fmaf(g[e, w],
 *                  positions[c, d], ..), one fmaf a step, both from +0; a NaN result is stored as 0x7fc00000.  Skipping a step with
 *                  g = +0 yields the same bits (the positions are finite, the chains start at +0: such a step adds +-0 and an
 *                  accumulator is never -0), so whether an implementation takes those steps is not part of the definition
 *   best           out_best[e] = the lowest w whose a[e, w] is the largest among those that are not NaN (-0 == +0); -1 for none
 *   location       moment / weight is the caller's: no division and no reciprocal on the device enters the definition
 *   positions      (n_cols, n_dims) float32 in C order on the host, one row per entry of cols; every entry finite
 *   outputs        out_amp (n_events, width) C order or null (the other outputs are the same bytes), out_weight (n_events),
 *                  out_moment (n_events, n_dims) C order, out_best (n_events).  One thread owns an event's chains from +0 to their
 *                  stores, no atomics: the same bytes whatever the call, its pieces, its slabs, the gap setting, the cache or the
 *                  device, and the bytes of the definition applied on the host to mts_waveforms' own snippets
 *   limits         T, width, n_events, taps, columns and the reference's columns as mts_waveforms; 1 <= n_dims <= MTS_LOCALIZE_MAX_DIMS
 *   chunks, chunk_status   as mts_waveforms; the results near a failed chunk are undefined
 * mts_localize: host cdata; cache_id 0 or a decoded-chunk cache, read in place and never inserted into, as mts_waveforms; the same
 * pieces (MTS_PIPE_BYTES) and slabs (MTS_WAVEFORMS_SLAB_BYTES, MTS_WAVEFORMS_GAP_ROWS).  The outputs are host memory.
 * mts_dev_localize: device d_cdata and d_* outputs on `device`; ev_row, ev_col0, positions and chunk_status on the host; no cache.
 * MTS_E_ARG with a message before anything is allocated or launched: what mts_waveforms refuses, a mode outside 0 .. 3, n_dims outside
 * the limit, no positions, a position that is not finite (its row and dimension are named), no out_weight, out_moment or out_best.
 * n_events == 0 is MTS_OK without a launch.
 */
int mts_localize(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                 const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                 long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                 const long *ev_row, const int *ev_col0, int before, int after, int width, int mode, int n_dims,
                 const float *positions /* (n_cols, n_dims) C order */, float *out_amp /* (n_events, width) or null */,
                 float *out_weight /* (n_events) */, float *out_moment /* (n_events, n_dims) */, int *out_best /* (n_events) */, int *chunk_status);

/*
 * Spatio-temporal template scores of filtered rows (an extension: the reference has no such call; its users pull Reader[...] across the
 * bus, filter it and run a matched filter on the host).  Only the scores cross the bus.  Everything is float32 and a definition, not a
 * tolerance:
 *   z              exactly mts_detect's z: the filter y[t, j] = sum_k taps[k] * x[t + half - k, cols[j]] (mts_decimate with q = 1 and
 *                  out_itemsize 4, bit for bit; x = 0 outside [valid_begin, valid_end)), and with reference 1 the float32 median over
 *                  all n_cols columns of row t subtracted (np.sort's order, NaN last, 0.5f * (a + b) for an even n_cols).  z[r, j] =
 *                  +0 for a row r outside [valid_begin, valid_end)
 *   templates      n_out templates of T rows x n_cols columns: floats on the host, (n_out, T, n_cols) C order, all finite; template
 *                  row `before` is laid on file row t, 0 <= before <= T
 *   score          score[t, k] = sum_tau sum_j z[t - before + tau, j] * K[k, tau, j] for row_begin <= t < row_end, formed as this
 *                  chain.  With n4 = n_cols rounded up to a multiple of 4, columns n_cols .. n4 - 1 of z and K are +0, and
 *                      acc = +0
 *                      for g in 0, 4, 8, .. < n4:              (column group, outermost)
 *                          for tau in 0 .. T - 1:
 *                              for j in g .. g + 3:
 *                                  acc = fmaf(z[t - before + tau, j], K[k, tau, j], acc)
 *                      score[t, k] = acc, or the bits 0x7fc00000 when acc is a NaN
 *                  Each (g, tau) is one v_mfma_f32_16x16x4_f32 step; the order does not depend on any tile size.  Zero template
 *                  entries are not skipped (inf * 0 is NaN); the sign and payload that float arithmetic gives a NaN differ from one
 *                  processor to the next and are not part of the definition.  float32 subnormals are kept, as operands and as
 *                  results.  score[t, k] depends on t, cols, taps, reference and template k alone: not on the other templates, the
 *                  tile, the slab, the piece, the call, the lane, cache residency, the entry point or the device.
 *   outputs        out (row_end - row_begin, n_out) float, C order
 *   limits         1 <= T <= MTS_CORRELATE_MAX_T; 1 <= n_out <= MTS_CORRELATE_MAX_OUT; 1 <= n_cols <= MTS_CORRELATE_MAX_COLS channel
 *                  indices, any order, repeats allowed; taps as mts_detect
 *                  Every call repacks the templates on the host (n4 * T * n_out rounded up to 64 floats: 12 MB for 128 templates of
 *                  61 x 385, 1 GiB at all three limits) and uploads them: a caller with many templates of many rows scores them in
 *                  several calls, or over fewer columns
 *   chunks         as mts_decimate: adjacent, ascending, covering [row_begin - before + half - n_taps + 1, row_end + T - before - 1 +
 *                  half) within [valid_begin, valid_end); valid_begin <= row_begin <= row_end <= valid_end.  row_begin == row_end is
 *                  MTS_OK with nothing written.
 *   chunk_status   MTS_CHUNK_* per chunk; the scores near a failed chunk are undefined
 * mts_correlate: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated piece by piece (MTS_PIPE_BYTES) in a
 * transient workspace and NOT inserted; a piece owns the rows of its chunks and a chunk in the halo of two pieces is inflated in
 * both.  Within a piece the rows go through the float workspace in slabs of at most 256 MiB (MTS_CORRELATE_SLAB_BYTES; never less than
 * one row and its T - 1 neighbours).  `out` is host memory.
 * mts_dev_correlate: device d_cdata and d_out on `device`; templates and chunk_status on the host; no cache.
 * MTS_E_ARG with a message before anything is allocated or launched: any argument outside the limits above, a template entry or a tap
 * that is not finite, no templates, no output buffer, a column outside [0, n_channels), chunks not adjacent or not covering the rows
 * read.
 */
int mts_correlate(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                  long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                  int before, int T, int n_out, const float *templates /* (n_out, T, n_cols) C order */,
                  float *out /* (row_end - row_begin, n_out) C order */, int *chunk_status);

/*
 * Template-matching events: the peaks of mts_correlate's scores, at most one per neighbourhood in time, each given to the template that
 * scored highest (an extension: the reference has no such call; its users pull the score matrix across the bus and pick its peaks on
 * the host).  Only the events cross the bus.  Everything is float32 and a definition, not a tolerance:
 *   score          score[t, k] is mts_correlate's, bit for bit, for the same templates, cols, before, taps and reference, for every
 *                  file row t of [valid_begin, valid_end): z is mts_detect's and +0 outside the recording, the fmaf chain runs from
 *                  +0 over column groups of 4, then tau, then the group's columns, a NaN is 0x7fc00000.  A row whose template window
 *                  reads nothing of the recording scores +0.
 *   event          (t, k) with row_begin <= t < row_end, score[t, k] > threshold[k] and no (t', k') that beats it: |t' - t| <=
 *                  exclude_rows, any template k', valid_begin <= t' < valid_end -- inside or outside [row_begin, row_end).  It beats
 *                  (t, k) when score[t', k'] > score[t, k], or they are equal and (t', k') precedes (t, k) in (row, template)
 *                  order.  mts_detect's words with every template a neighbour: a NaN score is no event and beats nothing; a plateau
 *                  gives one event, at its first row and lowest template; -0 equals +0; of two identical templates the lower index
 *                  has the event; a row has at most one event.  Calls on [a, b) and [b, c) together give the events of [a, c).
 *                  Equivalently: with b[t] the largest score of row t that is not a NaN and k*[t] the first template that attains
 *                  it, row t is an event when b[t] > threshold[k*[t]], no earlier row within exclude_rows has b >= b[t] and no later
 *                  one has b > b[t]; a row of NaNs has no b.
 *   threshold      n_out finite floats on the host, of any sign
 *   outputs        the events in ascending row order: out_row[i] = t (file row), out_template[i] = k, out_score[i] = the bits of
 *                  score[t, k].  *n_events: the events found, which may exceed max_events; then the first max_events of them are
 *                  written, nothing past them, and the call still answers MTS_OK (call again with room for *n_events).  max_events
 *                  0: a count, the outputs may be null.  The same bytes whatever the call, its pieces, its slabs, the cache, the
 *                  entry point or the device.
 *   limits         exclude_rows <= MTS_TMATCH_MAX_EXCLUDE; T, n_out, n_cols, taps and the reference as mts_correlate
 *   chunks         as mts_decimate: adjacent, ascending, covering [row_begin - exclude_rows - before + half - n_taps + 1, row_end +
 *                  exclude_rows + T - before - 1 + half) within [valid_begin, valid_end); valid_begin <= row_begin <= row_end <=
 *                  valid_end.  No chunks at all when that range is empty (every score near the rows is +0).  row_begin == row_end is
 *                  MTS_OK with *n_events = 0.
 *   chunk_status   MTS_CHUNK_* per chunk; the events near a failed chunk are undefined
 * mts_match_templates: host cdata; cache_id 0 or a decoded-chunk cache, used as mts_correlate uses it; nothing is inserted.  A piece
 * owns the rows of its chunks; within a piece the rows go through slabs of owned rows that keep both the float workspace (the owned
 * rows, exclude_rows either side and their T - 1 neighbours) and the score slab (the owned rows and exclude_rows either side, n_out
 * floats each) within 256 MiB (MTS_TMATCH_SLAB_BYTES; never less than one row with its neighbours): filter, median, k_correlate into
 * the score slab, then the row maxima, the event bitmap and its compaction.  The scores never leave the device.  The outputs are host
 * memory.
 * mts_dev_match_templates: device d_cdata and d_* outputs on `device`; templates, threshold, n_events and chunk_status on the host; no
 * cache.
 * MTS_E_ARG with a message before anything is allocated or launched: any argument outside the limits above, a template entry, a
 * threshold or a tap that is not finite, no templates, no thresholds, max_events < 0 or no output buffer for it, no n_events, a column
 * outside [0, n_channels), chunks not adjacent or not covering the rows read.
 */
int mts_match_templates(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                        const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags,
                        long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                        const int *cols, int reference, int before, int T, int n_out, const float *templates /* (n_out, T, n_cols) C order */,
                        const float *threshold /* n_out */, int exclude_rows, long max_events, long *out_row, int *out_template,
                        float *out_score, long *n_events, int *chunk_status);

/*
 * Template peeling: the filtered rows with matched templates subtracted, and the template events of those rows (an extension: the
 * reference has no such call; a template-matching sorter subtracts every matched template, scaled by its fitted amplitude, and
 * matches again -- a spike that overlaps a stronger one within exclude_rows is invisible to the first pass).  Everything is float32
 * and a definition, not a tolerance:
 *   z              mts_detect's / mts_correlate's z for cols, taps and reference: the filtered rows, minus the row median with
 *                  reference 1; defined for the file rows of [valid_begin, valid_end) only
 *   events         n_sub entries (sub_row[e], sub_tpl[e], sub_amp[e]) on the host: valid_begin <= sub_row[e] < valid_end,
 *                  non-decreasing in e (ties keep the caller's order), 0 <= sub_tpl[e] < n_out, sub_amp[e] finite.  Event e covers
 *                  file row t when 0 <= tau < T, tau = t - sub_row[e] + before.  n_sub == 0: the three pointers may be null
 *   residual       acc = z[t, j]; for every event e that covers t, in list order: acc = fmaf(-sub_amp[e], K[sub_tpl[e], tau, j], acc);
 *                  z'[t, j] = acc.  An event that does not cover the row issues no step (a masked step would turn a -0 into +0);
 *                  zero template entries are not skipped; rows outside the recording do not exist (mts_correlate's chain keeps
 *                  reading them as +0).  A NaN is stored as 0x7fc00000, with an empty list too; every other entry of an empty
 *                  list's result has z's bits.  z'[t, j] depends on t, cols[j], taps, reference and the events that cover t alone:
 *                  not on the other events, the tile, the slab, the piece, the call, the lane, cache residency, the entry point or
 *                  the device.  Calls on [a, b) and [b, c) together give the rows of [a, c).
 *   mts_residual   out (row_end - row_begin, n_cols) float, C order: z' of the file rows [row_begin, row_end)
 *   mts_match_residual   the events of mts_match_templates, for the same arguments, of the scores of z': score[t, k] is
 *                  mts_correlate's chain on z', bit for bit, for every file row t of [valid_begin, valid_end).  With n_sub == 0 not
 *                  one launch or byte differs from mts_match_templates.
 *   limits         n_sub <= 2^30; T, n_out, n_cols, taps and the reference as mts_correlate; exclude_rows, threshold, max_events and
 *                  the outputs as mts_match_templates
 *   chunks         mts_residual: as mts_decimate with q = 1, adjacent, ascending, covering [row_begin + half - n_taps + 1, row_end +
 *                  half) within [valid_begin, valid_end) -- the subtraction reads no row that the filter did not;
 *                  mts_match_residual: as mts_match_templates.  valid_begin <= row_begin <= row_end <= valid_end; row_begin ==
 *                  row_end is MTS_OK with nothing written.
 *   chunk_status   MTS_CHUNK_* per chunk; the rows and events near a failed chunk are undefined
 * mts_residual: host cdata; cache_id 0 or a decoded-chunk cache, used as mts_correlate uses it; nothing is inserted.  Within a piece
 * the rows go through the float workspace in slabs of at most 256 MiB of owned rows (MTS_RESIDUAL_SLAB_BYTES; never less than a row):
 * filter, median, then k_subtract -- a gather: every (row, column) belongs to one thread, which walks the events that cover its row
 * in list order; the events of a tile of rows are one range of the sorted list, found by binary search -- writes the slab's rows of
 * the output.  mts_match_residual runs the same kernel in place on mts_match_templates' z slab, between the median and k_correlate.
 * The events and a plain (n_out, T, n_cols) copy of the templates are uploaded only when n_sub > 0.  `out` is host memory.
 * mts_dev_residual, mts_dev_match_residual: device d_cdata and d_* outputs on `device`; templates, threshold, the events, n_events
 * and chunk_status on the host; no cache.
 * MTS_E_ARG with a message that names the offending entry, before anything is allocated or launched: as mts_correlate /
 * mts_match_templates, and an event out of row order, at a row outside [valid_begin, valid_end), with a template index outside [0,
 * n_out) or an amplitude that is not finite, n_sub outside [0, 2^30], or n_sub > 0 without the three arrays.
 */
int mts_residual(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                 const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                 long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                 int before, int T, int n_out, const float *templates /* (n_out, T, n_cols) C order */, long n_sub,
                 const long *sub_row /* n_sub */, const int *sub_tpl /* n_sub */, const float *sub_amp /* n_sub */,
                 float *out /* (row_end - row_begin, n_cols) C order */, int *chunk_status);
int mts_match_residual(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                       const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags,
                       long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                       const int *cols, int reference, int before, int T, int n_out, const float *templates /* (n_out, T, n_cols) C order */,
                       const float *threshold /* n_out */, int exclude_rows, long max_events, long n_sub, const long *sub_row /* n_sub */,
                       const int *sub_tpl /* n_sub */, const float *sub_amp /* n_sub */, long *out_row, int *out_template, float *out_score,
                       long *n_events, int *chunk_status);

/*
 * Per-channel power spectral density, Welch's method (an extension: the reference has no such call; its users run
 * scipy.signal.welch on Reader[...] on the host).  Only one float64 partial per (group, bin, column) crosses the bus.
 *   segments       segment s covers file rows [row_seg0 + s * step, row_seg0 + s * step + nperseg); the call computes segments
 *                  [seg_begin, seg_end): seg_begin is a multiple of the group size G, seg_end a multiple of G or the end of the
 *                  caller's range (the last group may then be short; not checked)
 *   nperseg, step  nperseg a power of two in [16, MTS_WELCH_MAX_NPERSEG]; 1 <= step <= nperseg
 *   taper          nperseg finite doubles on the host, rounded to the compute type
 *   detrend        1: subtract the segment's mean first (float64: integers' exact sum rounded once, floats' pairwise tree
 *                  v = v[0::2] + v[1::2]); 0: none
 *   csize          the FFT's compute type: 4 float, 8 double
 *   per segment and column: y[n] = F(double(x[n]) - mean) * F(taper[n]), X = real FFT of y in F (radix-4/2 Stockham passes
 *   over nperseg / 2 complex points, twiddles rounded once to F), P[k] = double(Re X[k])^2 + double(Im X[k])^2, k <= nperseg / 2.
 *   Blocks of B = MTS_WELCH_BLOCK_SEGMENTS segments are summed in segment order, groups of G segments (smallest multiple of B with
 *   G * step >= MTS_WELCH_GROUP_ROWS) in block order from +0, all in float64: the same bits whatever the call, its pieces, the
 *   launches or the device.  No scaling, no one-sided doubling, no division by the number of segments: the caller does that.
 *   out            (n_groups, nperseg / 2 + 1, n_cols) float64, C order, n_groups = ceil((seg_end - seg_begin) / G)
 *   chunks         as mts_decimate: adjacent, ascending, covering the rows of the segments; cols: n_cols >= 1, repeats allowed
 *   chunk_status   MTS_CHUNK_* per chunk; the partials of a segment that reads a failed chunk are undefined
 * mts_welch: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated piece by piece (MTS_PIPE_BYTES) in a
 * transient workspace and NOT inserted; pieces are cut at block boundaries, a chunk that blocks of two pieces read is inflated in
 * both, and the group sums are carried on the device from piece to piece.  `out` is host memory.
 * mts_dev_welch: device d_cdata and d_out on `device`, chunk_status on the host; no cache.
 * MTS_E_ARG before anything is launched: nperseg not a power of two in range, step outside [1, nperseg], a taper value that is not
 * finite, csize not 4 or 8, n_cols < 1, a column outside [0, n_channels), chunks not adjacent or not covering the rows read,
 * seg_begin not a multiple of G, seg_end <= seg_begin.
 */
int mts_welch(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
              const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_seg0,
              long seg_begin, long seg_end, int nperseg, long step, const double *taper, int detrend, int csize, int n_cols,
              const int *cols, double *out, int *chunk_status);

/*
 * Channel x channel Gram matrices and column sums per window (an extension: the reference has no such call; its users form
 * x.T @ x of Reader[...] on the host).  Only one partial per (group, column pair) crosses the bus.
 *   grid           the range [range_begin, range_end) in windows [range_begin + w * window_rows, min(.. + window_rows, range_end));
 *                  window w in groups of MTS_GRAM_GROUP_ROWS rows aligned to its start (the last may be short).  Groups are numbered
 *                  window after window: with K = ceil(window_rows / MTS_GRAM_GROUP_ROWS), group g is group g % K of window g / K.
 *                  The call computes groups [group_begin, group_end).
 *   the tree       a group is cut into slabs of MTS_GRAM_SLAB_ROWS rows aligned to its start (the last may be short).  Items are
 *                  converted to double once (exact but for 8-byte integers, which are rounded).  A slab's entry (i, j) is the chain of
 *                  v_mfma_f64_16x16x4_f64 steps over its rows 4 at a time in row order, from +0 (rows past the slab's end read as 0);
 *                  a group's entry is its slabs' entries added in slab order from +0, in double.  G[i, j] and G[j, i] are the same
 *                  value (one triangle, mirrored).  Nothing depends on chunks, calls, pieces, lanes, cache residency or the other
 *                  columns.  For an error bound: a product of a row goes through at most h = min(rows, SLAB) + slabs - 1 roundings
 *                  inside its group (a 4-row step rounds a term at most 4 times), plus the groups of the window on the host:
 *                  |G - sum x_i x_j| <= gamma_{h+3} * sum |x_i x_j| + n * 2^-1074 for a window of n rows.  The second term is the
 *                  underflow: float64 subnormals are kept, as operands and as results (the matrix cores do not flush them, and
 *                  the kernels are built with hipcc's default float mode, which keeps them elsewhere), so a product that lands
 *                  below 2^-1022 is rounded to a multiple of 2^-1074, an absolute error of at most 2^-1075 that no relative
 *                  term covers; sums inside the subnormal range are exact; n products, each scaled by less than 2 by the later
 *                  roundings.  Items k * 2^e whose products and sums are exactly representable, subnormal or not, give exact
 *                  entries.
 *                  Column sums: per slab, the items added in row order from 0 (integers: int64 modulo 2^64; floats: double from +0),
 *                  slabs in slab order.
 *   out_gram       (group_end - group_begin, n_cols, n_cols): int64 for 1- and 2-byte integers (exact: a group's sum of products is
 *                  an integer below 2^52), float64 for every other type
 *   out_sum        (group_end - group_begin, n_cols): int64 for every integer type (numpy's wrap modulo 2^64, so that the host's
 *                  sums equal np.sum(x, dtype=np.int64)), float64 for floats
 *   chunks         as mts_decimate: adjacent, ascending, covering the groups' rows; cols: 1 <= n_cols <= MTS_GRAM_MAX_COLS, repeats
 *                  allowed
 *   chunk_status   MTS_CHUNK_* per chunk; the partials of a group that reads a failed chunk are undefined
 * mts_gram: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated piece by piece (MTS_PIPE_BYTES) in a
 * transient workspace and NOT inserted; pieces are cut at group boundaries, a chunk that groups of two pieces read is inflated in both.
 * out_gram / out_sum are host memory.
 * mts_dev_gram: device d_cdata, d_gram and d_sum on `device`, chunk_status on the host; no cache.
 * MTS_E_ARG before anything is launched: n_cols < 1 or too many, a column outside [0, n_channels), window_rows < 1, an empty or
 * negative range, a group run that is empty or outside the range, chunks not adjacent, empty or not covering the groups' rows.
 */
int mts_gram(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
             const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long range_begin,
             long range_end, long window_rows, long group_begin, long group_end, int n_cols, const int *cols, void *out_gram, void *out_sum,
             int *chunk_status);

/*
 * The same Gram matrices and column sums over the filtered signal z of mts_detect instead of the decoded items (an extension, as
 * mts_gram): what Reader.cov forms when taps= or reference= is given, the covariance a spike sorter whitens with.  By definition the
 * result is mts_gram of a float32 recording whose items are z.
 *   z              mts_detect's: the chunks (adjacent), valid_begin .. reference and chunk_status are those of mts_detect.  z[t, j] is
 *                  float32, the FIR of the selected columns with x = 0 outside [valid_begin, valid_end), minus, with reference 1, the
 *                  row's median over them.  The arguments are checked as mts_detect checks them; with a reference n_cols <=
 *                  MTS_DETECT_MAX_REF_COLS, without one n_cols <= MTS_GRAM_MAX_COLS.  z never leaves the device: it is made z slab by
 *                  z slab (at most MTS_ZGRAM_SLAB_BYTES of float32, default 256 MiB, rounded down to whole slabs of
 *                  MTS_GRAM_SLAB_ROWS rows and never less than one) and reduced where it lies.
 *   grid           range_begin, range_end, window_rows, group_begin, group_end as mts_gram, inside [valid_begin, valid_end): the
 *                  windows, the groups of MTS_GRAM_GROUP_ROWS rows and their numbering are mts_gram's
 *   the tree       mts_gram's, word for word: a group is cut into slabs of MTS_GRAM_SLAB_ROWS rows aligned to its start; the items
 *                  are widened to double once (exact); a slab's entry (i, j) is the chain of v_mfma_f64_16x16x4_f64 steps over its
 *                  rows 4 at a time in row order, from +0 (rows past the slab's end read as 0); a group's entry is its slabs' entries
 *                  added in slab order from +0; one triangle is mirrored.  Column sums: per slab, the items added in row order in
 *                  double from +0, slabs in slab order.  The error bound of mts_gram holds with z for x.  The result is the same
 *                  bits whatever the lanes, calls, pieces, z slabs and cache residency.  Unlike mts_gram it is NOT independent of
 *                  the column set when reference is 1: the median is taken over the selected columns, so another set is another z.
 *                  A NaN in a row of x makes, with reference 1, every item of that row of z NaN.
 *   out_gram       (group_end - group_begin, n_cols, n_cols) float64
 *   out_sum        (group_end - group_begin, n_cols) float64
 *   chunks         adjacent, covering the filter support of the call's groups: with [lo, hi) the rows of groups [group_begin,
 *                  group_end) and half = (n_taps - 1) / 2, the rows [lo + half - (n_taps - 1), hi + half) inside the valid range
 * When a chunk of the call did not decode, chunk_status says so and the outputs are to be discarded.
 * mts_filtered_gram: host cdata and outputs; cache_id 0 or a decoded-chunk cache, resident chunks are read where they lie and
 * nothing is inserted; pieces (MTS_PIPE_BYTES) are cut at group boundaries.  mts_dev_filtered_gram: device d_cdata, d_gram and d_sum;
 * the small arrays on the host; no cache.
 * MTS_E_ARG before anything is allocated or launched: what mts_detect refuses of its filter arguments, what mts_gram refuses of the
 * grid, a range outside the valid rows, or chunks that do not cover the support.
 */
int mts_filtered_gram(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                      const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long valid_begin,
                      long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long range_begin, long range_end,
                      long window_rows, long group_begin, long group_end, double *out_gram, double *out_sum, int *chunk_status);

/*
 * One round of a radix select over the windows of mts_window_stats (an extension: the reference has no such call; its users sort
 * Reader[...] on the host).  Order statistics do not combine across chunks; digit histograms of candidates do.  Only the histograms
 * cross the bus.  The range, the windows, the chunks (ascending, not necessarily adjacent), cols, flags and chunk_status are those of
 * mts_window_stats.
 *   order key      a u64 with key_bits significant bits whose unsigned order is np.sort's order of the items:
 *                    mode 0  the item in its own type, key_bits = 8 * itemsize.  Unsigned integers: the value.  Signed integers: the
 *                            two's-complement pattern with the sign bit flipped.  Floats: with b the bit pattern and SIGN its top bit,
 *                            a NaN of either sign -> all ones; -0 and +0 -> SIGN (one key); b & SIGN ? ~b : b | SIGN otherwise.
 *                            All ones is the key of a NaN and of nothing else (+inf is below it).
 *                    mode 1  the double d = double(x) - center[w, j] (one IEEE subtraction), mapped as a float; key_bits = 64
 *                    mode 2  the double |d|, mapped the same way; key_bits = 64
 *                  center: (n_windows, n_cols) doubles on the host, read in modes 1 and 2 only (may be NaN or infinite)
 *   digits         MTS_RANK_BITS = 8 bits wide
 *   selectors      MTS_RANK_SELECTORS = 2 per (window, column) cell: sel_shift (n_windows, 2, n_cols) ints and sel_prefix of the same
 *                  shape, u64, on the host.  shift < 0: the selector is inactive.  Otherwise 0 <= shift <= key_bits - 8, and the
 *                  selector's candidates are the cell's items with key >> (shift + 8) == prefix (every item when shift + 8 ==
 *                  key_bits: the prefix must then be 0; a prefix must fit the key_bits - shift - 8 bits above the digit).  The two
 *                  selectors of a cell are counted independently; a caller that wants every item counted once keeps their
 *                  candidate sets disjoint.
 *   outputs        hist  (n_windows, 2, 256, n_cols) u32: the number of candidates with (key >> shift) & 255 == digit (exact while a
 *                        window has fewer than 2^32 rows)
 *                  kmin, kmax  (n_windows, 2, n_cols) u64: the smallest and the largest candidate key; all ones and 0 when there
 *                        is no candidate (and for an inactive selector)
 *                  count (n_windows) rows of the window held by the chunks that decoded
 *                  All of them are integers accumulated with integer atomics: counts add, kmin / kmax combine with min / max.  A
 *                  caller that splits a window over calls, pieces or lanes combines the outputs in any order and gets the same bits.
 * mts_rank_hist: host cdata; cache_id 0 or a decoded-chunk cache.  A chunk resident there (whole rows) is read where it lies --
 * c_lengths[i] may then be 0 (MTS_E_MISS when it is not resident).  The others are inflated (whole chunks, adler32 checked) and
 * counted piece by piece in a transient workspace, the compressed bytes of the next piece crossing the bus beside the kernels; they
 * are NOT inserted into the cache.  Outputs are host memory.
 * mts_dev_rank_hist: device d_cdata and d_* outputs on `device`; selectors, center, count and chunk_status on the host; no cache.
 * MTS_E_ARG before anything is launched: what mts_window_stats refuses, a mode outside 0..2, no center in modes 1 and 2, a shift
 * above key_bits - 8, or a prefix that does not fit.
 */
#define MTS_RANK_BITS 8
#define MTS_RANK_SELECTORS 2
int mts_rank_hist(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                  const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags, long row_begin,
                  long row_end, long window_rows, int n_cols, const int *cols, int mode, const double *center,
                  const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *out_hist, unsigned long long *out_kmin,
                  unsigned long long *out_kmax, long *out_count, int *chunk_status);

/*
 * The same round over the filtered signal z of mts_detect instead of the decoded items (an extension, as mts_rank_hist): what
 * Reader.quantile / median / mad order when taps= or reference= is given.  The chunks (adjacent), valid_begin .. reference and
 * chunk_status are those of mts_detect: z[t, j] is float32, the FIR of the selected columns inside [valid_begin, valid_end) minus, with
 * reference 1, the row's median over them.  z never leaves the device: it is made slab by slab (at most MTS_ZRANK_SLAB_BYTES of
 * float32, default 256 MiB) and counted where it lies.
 *   items          the float32 z[t, j]: mode, center, the order key (key_bits = 32 in mode 0, 64 in modes 1 and 2), the digits and the
 *                  selectors are mts_rank_hist's for a float32 recording
 *   grid           row_begin, row_end, window_rows as mts_rank_hist, inside [valid_begin, valid_end): window w is the rows
 *                  [row_begin + w * window_rows, min(row_end, row_begin + (w + 1) * window_rows))
 *   count range    row_begin <= count_begin <= count_end <= row_end.  Only the rows of [count_begin, count_end) are counted, so that a
 *                  caller cuts a grid over calls wherever it likes and adds the partials; the chunks cover the filter's support of
 *                  the count range, [count_begin + half - (n_taps - 1), count_end + half) inside the valid range, half = (n_taps - 1) / 2
 *   outputs        hist, kmin, kmax of mts_rank_hist's shapes for the grid, zeroed / initialised once per call and accumulated with
 *                  integer atomics across slabs and pieces: the same bits whatever the slabs, pieces, calls and cache residency.
 *                  count (n_windows): the rows of window w inside the count range
 * When a chunk of the call did not decode, chunk_status says so and the outputs are to be discarded (as the events of mts_detect).
 * mts_filtered_rank_hist: host cdata and outputs; cache_id 0 or a decoded-chunk cache, resident chunks are read where they lie and
 * nothing is inserted.  mts_dev_filtered_rank_hist: device d_cdata and d_* outputs; the small arrays on the host; no cache.
 * MTS_E_ARG before anything is allocated or launched: what mts_detect refuses of its filter arguments, what mts_rank_hist refuses of
 * mode, center and the selectors (key_bits of a float32 item), a grid outside the valid range, a count range outside the grid, or
 * chunks that do not cover the support.
 */
int mts_filtered_rank_hist(int device, long cache_id, int n_chunks, const long *chunk_keys, const long *chunk_row0, const unsigned char *cdata,
                           const long *c_offsets, const long *c_lengths, const long *n_rows, int n_channels, int itemsize, int flags,
                           long valid_begin, long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                           long row_begin, long row_end, long window_rows, long count_begin, long count_end, int mode, const double *center,
                           const unsigned long long *sel_prefix, const int *sel_shift, unsigned int *out_hist, unsigned long long *out_kmin,
                           unsigned long long *out_kmax, long *out_count, int *chunk_status);

/* ---------------------------------------------------------------------------------------------
 * Device-resident variants (inputs and outputs already in HBM; used by bench.py and by callers that
 * keep recordings on the GPU).  Pointers are device pointers on `device`; `stream` is a hipStream_t
 * (0 = default stream).  The small index arrays stay on the host.  Not part of the drop-in.
 * ------------------------------------------------------------------------------------------- */
int mts_dev_compress_chunks(int device, void *stream, const void *d_raw, int n_channels, int itemsize,
                            const long *chunk_bounds, int n_chunks, int flags, int level,
                            unsigned char *d_out, const long *out_slot_offsets /* 16-B aligned */,
                            long *out_sizes /* host; valid when the call returns */);
/* Chunk i is written at d_out + out_offsets[i].  That address must be a multiple of `itemsize`; any such offset is allowed (chunks
 * back to back, no other alignment: the kernel stores 16 bytes, dwords or single items as the address permits, and never a byte
 * outside the chunk's n_rows[i] * n_channels * itemsize bytes).  An address that is not returns MTS_E_ARG, with a message naming
 * the chunk, before anything is launched.  A chunk whose status is not MTS_CHUNK_OK leaves its bytes of d_out untouched. */
int mts_dev_decompress_chunks(int device, void *stream, const unsigned char *d_cdata,
                              const long *c_offsets, const long *c_lengths, const long *n_rows,
                              int n_chunks, int n_channels, int itemsize, int flags, void *d_out,
                              const long *out_offsets, int *chunk_status /* host */);
int mts_dev_window_stats(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets,
                         const long *c_lengths, const long *chunk_row0, const long *n_rows, int n_chunks,
                         int n_channels, int itemsize, int flags, long row_begin, long row_end, long window_rows,
                         int n_cols, const int *cols, void *d_min, void *d_max, void *d_sum, void *d_sumsq,
                         long *count /* host */, int *chunk_status /* host */);
int mts_dev_decimate(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets,
                     const long *c_lengths, const long *chunk_row0, const long *n_rows, int n_chunks,
                     int n_channels, int itemsize, int flags, long valid_begin, long valid_end, long first_row,
                     long n_out, int q, int n_taps, const double *taps, int out_itemsize, int n_cols,
                     const int *cols, void *d_out, int *chunk_status /* host */);
int mts_dev_project(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                    const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin,
                    long row_end, int n_cols, const int *cols, const double *offset /* host */, int n_out, const double *weights /* host */,
                    int out_itemsize, void *d_out, int *chunk_status /* host */);
int mts_dev_detect(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                   const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                   long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols,
                   const float *threshold /* host */, int sign, int reference, int exclude_rows, int exclude_cols, long max_events,
                   long *d_row, int *d_pos, float *d_amp, long *n_events /* host */, int *chunk_status /* host */);
int mts_dev_waveforms(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                      const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                      long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                      const long *ev_row /* host */, const int *ev_col0 /* host */, int before, int after, int width,
                      float *d_wave /* (n_events, T, width) C order or null */, float *d_min, int *d_argmin, float *d_max, int *d_argmax,
                      int *chunk_status /* host */);
int mts_dev_mean_waveforms(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                           const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                           long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                           const long *ev_row /* host */, const int *ev_col0 /* host */, const int *ev_label /* host */, int n_labels, int before,
                           int after, int width, double resolution, long long *d_sum, int *d_count, long *d_skipped, int *chunk_status /* host */);
int mts_dev_waveform_features(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                              const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                              long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                              const long *ev_row /* host */, const int *ev_col0 /* host */, int before, int after, int width, int n_comp,
                              const float *basis /* host */, float *d_feat, int *chunk_status /* host */);
int mts_dev_localize(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                     const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                     long valid_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference, long n_events,
                     const long *ev_row /* host */, const int *ev_col0 /* host */, int before, int after, int width, int mode, int n_dims,
                     const float *positions /* host */, float *d_amp /* or null */, float *d_weight, float *d_moment, int *d_best,
                     int *chunk_status /* host */);
int mts_dev_correlate(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                      const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                      long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                      int before, int T, int n_out, const float *templates /* host */, float *d_out, int *chunk_status /* host */);
int mts_dev_match_templates(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                            const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                            long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                            const int *cols, int reference, int before, int T, int n_out, const float *templates /* host */,
                            const float *threshold /* host */, int exclude_rows, long max_events, long *d_row, int *d_template,
                            float *d_score, long *n_events /* host */, int *chunk_status /* host */);
int mts_dev_residual(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                     const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                     long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols, const int *cols, int reference,
                     int before, int T, int n_out, const float *templates /* host */, long n_sub, const long *sub_row /* host */,
                     const int *sub_tpl /* host */, const float *sub_amp /* host */, float *d_out, int *chunk_status /* host */);
int mts_dev_match_residual(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                           const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                           long valid_begin, long valid_end, long row_begin, long row_end, int n_taps, const double *taps, int n_cols,
                           const int *cols, int reference, int before, int T, int n_out, const float *templates /* host */,
                           const float *threshold /* host */, int exclude_rows, long max_events, long n_sub, const long *sub_row /* host */,
                           const int *sub_tpl /* host */, const float *sub_amp /* host */, long *d_row, int *d_template, float *d_score,
                           long *n_events /* host */, int *chunk_status /* host */);
int mts_dev_welch(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                  const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_seg0,
                  long seg_begin, long seg_end, int nperseg, long step, const double *taper, int detrend, int csize, int n_cols,
                  const int *cols, double *d_out, int *chunk_status /* host */);
int mts_dev_gram(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths, const long *chunk_row0,
                 const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long range_begin, long range_end, long window_rows,
                 long group_begin, long group_end, int n_cols, const int *cols, void *d_gram, void *d_sum, int *chunk_status /* host */);
int mts_dev_rank_hist(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                      const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long row_begin,
                      long row_end, long window_rows, int n_cols, const int *cols, int mode, const double *center /* host */,
                      const unsigned long long *sel_prefix /* host */, const int *sel_shift /* host */, unsigned int *d_hist,
                      unsigned long long *d_kmin, unsigned long long *d_kmax, long *count /* host */, int *chunk_status /* host */);
int mts_dev_filtered_gram(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                          const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags, long valid_begin,
                          long valid_end, int n_taps, const double *taps /* host */, int n_cols, const int *cols /* host */, int reference,
                          long range_begin, long range_end, long window_rows, long group_begin, long group_end, double *d_gram, double *d_sum,
                          int *chunk_status /* host */);
int mts_dev_filtered_rank_hist(int device, void *stream, const unsigned char *d_cdata, const long *c_offsets, const long *c_lengths,
                               const long *chunk_row0, const long *n_rows, int n_chunks, int n_channels, int itemsize, int flags,
                               long valid_begin, long valid_end, int n_taps, const double *taps /* host */, int n_cols,
                               const int *cols /* host */, int reference, long row_begin, long row_end, long window_rows, long count_begin,
                               long count_end, int mode, const double *center /* host */, const unsigned long long *sel_prefix /* host */,
                               const int *sel_shift /* host */, unsigned int *d_hist, unsigned long long *d_kmin,
                               unsigned long long *d_kmax, long *count /* host */, int *chunk_status /* host */);
/* integer-exact synthetic recording, rows [t0, t1) of n_channels int16, on device */
int mts_dev_synth_int16(int device, void *stream, void *d_out, long t0, long t1, int n_channels,
                        long seed);

/* Device memory for callers of the dev_* entry points (bench.py, the tests at BASELINE's sizes): allocate, copy and wait through
 * THIS library, so that a process holds its recordings with the HIP runtime the kernels are launched with and needs no other
 * (torch ships its own runtime libraries).  kind: 0 host -> device, 1 device -> host, 2 device -> device; mts_dev_copy returns
 * when the copy is done.  mts_dev_compare: bytes that differ between two device buffers (16-byte aligned) and the first such offset
 * (-1: none) -- the round-trip check of a recording that stays in HBM. */
/* Page-locked host memory (hipHostMalloc): the host entry points copy to / from such a buffer by DMA directly, without the pinned
 * pieces and host copies that pageable memory needs (Reader.tofile decodes into two of these and writes the file from them). */
int mts_host_alloc(long nbytes, void **h_ptr);
int mts_host_free(void *h_ptr);
int mts_dev_alloc(int device, long nbytes, void **d_ptr);
int mts_dev_free(int device, void *d_ptr);
int mts_dev_copy(int device, void *stream, void *dst, const void *src, long nbytes, int kind);
int mts_dev_sync(int device);               /* hipDeviceSynchronize on `device` */
int mts_dev_compare(int device, void *stream, const void *d_a, const void *d_b, long nbytes, long *n_diff, long *first_diff);

/* Kernel-stage timings (ms, HIP events on the launch stream) of the last dev_* call on `device`:
 * fills up to `cap` entries of (name, ms); returns the number of stages.  For bench.py / profiling. */
int mts_last_stage_times(int device, const char **names, float *ms, int cap);

/* What the last successful mts_waveforms / mts_dev_waveforms (or mts_mean_waveforms / mts_dev_mean_waveforms, mts_waveform_features / mts_dev_waveform_features, mts_localize / mts_dev_localize) call on `device` did, for the tests and the benchmark: out[0] its pieces,
 * out[1] its slabs, out[2] the slabs among them that were begun at a gap, out[3] the microseconds of its gather kernels (measured,
 * with a wait per slab, only while MTS_WAVEFORMS_TIME is set; else 0). */
int mts_waveforms_last_plan(int device, long *out /* 4 */);

/* Debug/parity taps for the GPU tests (stage-by-stage comparison with the oracle); host buffers. */
int mts_debug_match_tables(int device, const void *stream_bytes, long n, int level,
                           unsigned *t_full, unsigned *t_quarter);
int mts_debug_tokens(int device, const void *stream_bytes, long n, int level,
                     unsigned short *tokens /* (dist, lc) pairs, capacity n+1 */, long *n_tokens);
int mts_debug_deflate(int device, const void *stream_bytes, long n, int level, unsigned char *out,
                      long out_cap, long *out_len);
int mts_debug_inflate(int device, const unsigned char *zbytes, long zlen, unsigned char *out,
                      long out_cap, long *out_len, int *status);

/* release every device allocation held by the library (workspaces are otherwise cached) */
void mts_release(void);

#ifdef __cplusplus
}
#endif
#endif
