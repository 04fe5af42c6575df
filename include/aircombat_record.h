/* aircombat_record.h -- C ABI of the device flight recorder: what a Tacview ACMI frame needs, captured on the device after every step
 * of a handle, for a chosen set of envs, into a ring of frames in HBM.
 *
 * BaseEnv.render (R/envs/JSBSim/envs/env_base.py:207-250; R = the reference repository) writes one ACMI frame per call from the
 * simulators' log() messages, which here means ac_get_entity per aircraft, ac_get_state for the step counter and the chaff bookkeeping,
 * and ac_get_missile per munition slot, from Python after every step. A recorder takes the same values with one small kernel per step,
 * queued by the library itself behind the step's own launches, so the steps of ac_rollout_collect, ac_share_rollout_collect and
 * ac_eval_run (which never return to Python) are recorded like any other. Same library as aircombat.h (libaircombat_hip.so), same
 * errors: 0 on success, -1 on failure with the message in ac_last_error() and nothing changed. One caller thread per handle.
 *
 * Selection: a sorted, duplicate-free list of S env indices of the handle (NULL: all E). Capacity: F frames. Every capture is queued by
 * a host call, so the frame count is a host integer: capture c goes to slot c % F, and frames [max(0, count - F), count) are readable.
 *
 * Per aircraft and frame (ac_recorder_layout gives the table; nothing else states offsets):
 *   cur_step    int32        the aircraft's step counter (ac_get_state's cur_step)
 *   flags       int32        bit 0 (AC_REC_DONE): the aircraft's done byte of the step just taken (0 in a frame taken after a reset);
 *                            bit 1 (AC_REC_AFTER_RESET): the frame was taken after a reset
 *   status      int32        the aircraft's status (AC_ALIVE ...)
 *   entity      12 float64   ac_get_entity's twelve values, bit for bit
 *   msl_status  K int32      per munition slot k < K = msl_slots: ac_get_missile's out[0]
 *   msl_model   K int32      ac_get_missile's out[11] (0 AIM-9L, 1 AIM-120B, 2 AIM-9M)
 *   msl_pose    5 K float64  slot-major: px, py, pz, theta, psi as ac_get_missile reports them
 *   ext         2 int32      the scenario tasks' two packed extension words (chaff bookkeeping among them); only where the handle has them
 * A column without elements (K = 0, no extension) is absent from the table.
 *
 * The ring is field-major: column c with `count` elements per aircraft is the array [F][count][S * A] of its element type, lane
 * index = (position of the env in the selection) * A + agent, so every store of a capturing wave is contiguous. Columns start at
 * multiples of 256 bytes.
 *
 * Hooks. The recorder attached to a handle is captured behind every step the handle takes (ac_step, ac_step_host*, ac_step_async_device,
 * ac_step_timed_device, and the steps queued by the three collectors) and, with AC_REC_AFTER_RESET, behind ac_reset. A handle with a
 * recorder attached takes its host steps through HIP launches instead of the AQL queue. With nothing attached every path dispatches
 * exactly as it does without this header.
 */
#ifndef AIRCOMBAT_RECORD_H
#define AIRCOMBAT_RECORD_H
#include <stdint.h>
#include "aircombat.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ac_recorder ac_recorder_t;
enum { AC_REC_DONE = 1, AC_REC_AFTER_RESET = 2, AC_REC_MAX_COLUMNS = 8, AC_REC_NAME_LEN = 16 };

typedef struct {
  char name[16];                 /* AC_REC_NAME_LEN */
  int32_t elem_size;             /* 4 (int32) or 8 (float64) */
  int32_t count;                 /* elements per aircraft and frame */
} ac_recorder_column_t;
typedef struct {
  int32_t n_columns;
  int32_t bytes_per_aircraft_frame;
  ac_recorder_column_t columns[8];   /* AC_REC_MAX_COLUMNS */
} ac_recorder_layout_t;
/* The column table of a handle of that shape (no GPU, no handle): task is an AC_TASK_* value, A = aircraft per env (1 .. 8),
 * msl_slots = munition slots per aircraft (0 .. 4), has_ext != 0 where the handle keeps the scenario extension. */
int ac_recorder_layout(int32_t task, int32_t A, int32_t msl_slots, int32_t has_ext, ac_recorder_layout_t* out);

/* sel: S sorted, duplicate-free env indices in [0, E), or NULL for all envs (S is then ignored). 1 <= S <= E, F >= 1. The ring starts
 * zeroed. The handle must outlive its recorders; ac_destroy disables the attached one, which then refuses everything but ac_recorder_destroy. */
int ac_recorder_create(ac_env_t* env, const int32_t* sel, int32_t S, int32_t F, ac_recorder_t** out);
int ac_recorder_destroy(ac_recorder_t* rec);   /* detaches it first where it is attached */
/* device bytes a recorder of that shape allocates: the ring, an explicit selection and the staging buffer of ac_recorder_read */
int ac_recorder_bytes(ac_env_t* env, int32_t S, int32_t F, int64_t* bytes);
/* One attached recorder per handle: a second attach, and a recorder made for another handle, are refused. */
int ac_recorder_attach(ac_env_t* env, ac_recorder_t* rec);
int ac_recorder_detach(ac_env_t* env);         /* nothing attached: not an error */
/* An explicit capture of the handle's state as it is on its stream now, on any recorder, attached or not. */
int ac_recorder_capture(ac_recorder_t* rec, int32_t after_reset);
int64_t ac_recorder_count(ac_recorder_t* rec); /* frames captured so far (-1: null handle) */

typedef struct {
  int32_t task, A, msl_slots, has_ext;
  int32_t E, S, F, attached;
  int64_t count, bytes;
} ac_recorder_info_t;
int ac_recorder_info(ac_recorder_t* rec, ac_recorder_info_t* out);

/* Frames [f0, f0 + n) of one selected env, packed on the device into a staging buffer and copied to host_out in one copy (waits for
 * the handle's stream): the layout's columns in order, column c as [n][count][A] of its element type, nothing between the columns
 * (n * A * bytes_per_aircraft_frame bytes in all). Refused: an env that is not selected, n < 1, frames already overwritten
 * (f0 < count - F) or not yet captured (f0 + n > count). */
int ac_recorder_read(ac_recorder_t* rec, int32_t env, int64_t f0, int32_t n, void* host_out);
/* Column `column` of the ring in device memory, [F][count][S * A] elements (`elements` in all), valid while the recorder lives. Captures
 * are written on the handle's stream (ac_stream): order reads after it. */
int ac_recorder_device_ptr(ac_recorder_t* rec, int32_t column, void** ptr, int64_t* elements);

#ifdef __cplusplus
}
#endif
#endif
