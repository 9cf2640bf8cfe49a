/* mrcal_amd: MI355X-native implementation of mrcal's optimize() /
 * optimizer_callback() hot path. C ABI of libmrcal_amd.so.
 *
 * Two tiers of entry points:
 *
 * 1. DROP-IN TIER. Same names, argument order, argument meaning and error
 *    behaviour as the functions the reference's Python wrapper (and any ctypes
 *    harness) binds for this path. A process that dlopen()s libmrcal_amd.so
 *    instead of libmrcal.so and calls these gets the GPU implementation. All
 *    pointers are HOST pointers, the caller allocates every buffer, sizes are
 *    in bytes where the reference says bytes. Each declaration cites the
 *    reference interface it replaces (file:line in dkogan/mrcal).
 *
 * 2. RESIDENT TIER (mrcal_amd_*). The same computation with the problem held
 *    in HBM across calls: create a problem once, then evaluate / step / solve
 *    without any host<->device traffic beyond scalars. This is what the
 *    benchmark and the multi-GPU driver use. No reference counterpart: the
 *    reference has no device.
 *
 * No torch types, no C++ types: plain pointers and sizes only.
 */
#pragma once
#include <stdint.h>
#include <stdbool.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Types. Binary-compatible with the reference's (types.h, basic-geometry.h) */
/* ------------------------------------------------------------------------ */

/* reference: types.h:105-127 (mrcal_lensmodel_type_t). Same numeric values */
typedef enum
{
    MRCAL_LENSMODEL_INVALID               = -2,
    MRCAL_LENSMODEL_INVALID_BADCONFIG     = -1,
    MRCAL_LENSMODEL_INVALID_MISSINGCONFIG = -3,
    MRCAL_LENSMODEL_INVALID_TYPE          = -4,
    MRCAL_LENSMODEL_PINHOLE               = 0,
    MRCAL_LENSMODEL_STEREOGRAPHIC         = 1,
    MRCAL_LENSMODEL_LONLAT                = 2,
    MRCAL_LENSMODEL_LATLON                = 3,
    MRCAL_LENSMODEL_OPENCV4               = 4,
    MRCAL_LENSMODEL_OPENCV5               = 5,
    MRCAL_LENSMODEL_OPENCV8               = 6,
    MRCAL_LENSMODEL_OPENCV12              = 7,
    MRCAL_LENSMODEL_CAHVOR                = 8,
    MRCAL_LENSMODEL_CAHVORE               = 9,
    MRCAL_LENSMODEL_SPLINED_STEREOGRAPHIC = 10
} mrcal_lensmodel_type_t;

/* reference: types.h:131-145 (mrcal_lensmodel_t): 16 bytes, the
   configuration union sits at offset 8 */
typedef struct
{
    mrcal_lensmodel_type_t type;
    union
    {
        struct { double   linearity;               } LENSMODEL_CAHVORE__config;
        struct { uint16_t order, Nx, Ny, fov_x_deg; } LENSMODEL_SPLINED_STEREOGRAPHIC__config;
    };
} mrcal_lensmodel_t;

/* reference: basic-geometry.h:60-91 */
typedef union { struct { double x,y;   }; double xy[2];  } mrcal_point2_t;
typedef union { struct { double x,y,z; }; double xyz[3]; } mrcal_point3_t;
typedef struct { mrcal_point3_t r, t; }                    mrcal_pose_t;

/* reference: types.h:139-148 */
typedef union { struct { double x2, y2; }; double values[2]; } mrcal_calobject_warp_t;

/* reference: types.h:195-263 */
typedef struct { int intrinsics; int extrinsics; /* -1: at the reference */ } mrcal_camera_index_t;
typedef struct { mrcal_camera_index_t icam; int iframe;  } mrcal_observation_board_t;
typedef struct { mrcal_camera_index_t icam; int i_point; } mrcal_observation_point_t;
typedef struct
{
    mrcal_camera_index_t icam;
    bool                 last_in_set : 1;
    bool                 outlier     : 1;
    mrcal_point3_t       px; /* UNPROJECTED observation vector */
} mrcal_observation_point_triangulated_t;

/* reference: types.h:283-307. One byte, passed BY VALUE. Bit order matters */
typedef struct
{
    bool do_optimize_intrinsics_core         : 1;
    bool do_optimize_intrinsics_distortions  : 1;
    bool do_optimize_extrinsics              : 1;
    bool do_optimize_frames                  : 1;
    bool do_optimize_calobject_warp          : 1;
    bool do_apply_regularization             : 1;
    bool do_apply_outlier_rejection          : 1;
    bool do_apply_regularization_unity_cam01 : 1;
} mrcal_problem_selections_t;

/* reference: types.h:313-315 (empty in the reference, kept as a placeholder) */
typedef struct { char _unused; } mrcal_problem_constants_t;

/* reference: types.h:321-344 */
typedef struct
{
    double rms_reproj_error__pixels; /* <0: failure */
    int    Noutliers_board;
    int    Noutliers_triangulated_point;
} mrcal_stats_t;

/* The slice of SuiteSparse's cholmod_sparse that the reference's callback
   touches (mrcal.c:4461-4463: p, i, x only). Field order as in CHOLMOD so
   that a caller holding a real cholmod_sparse can pass it as is. Jt is
   (Nstate x Nmeasurements) compressed-column, i.e. J in CSR.
   A translation unit that also includes SuiteSparse's <cholmod.h> (or
   libdogleg's <dogleg.h>, which does) defines MRCAL_AMD_HAVE_CHOLMOD_SPARSE
   first and gets the real type */
#ifndef MRCAL_AMD_HAVE_CHOLMOD_SPARSE
struct cholmod_sparse_struct
{
    size_t nrow, ncol, nzmax;
    void *p, *i, *nz, *x, *z;
    int stype, itype, xtype, dtype, sorted, packed;
};
#endif

/* ------------------------------------------------------------------------ */
/* DROP-IN TIER                                                              */
/* ------------------------------------------------------------------------ */

/* reference: mrcal.c:165-253 / mrcal.h (lens model names) */
bool        mrcal_lensmodel_from_name(mrcal_lensmodel_t* lensmodel, const char* name);
bool        mrcal_lensmodel_name     (char* out, int size, const mrcal_lensmodel_t* lensmodel);
/* reference: mrcal.c:303-335 */
int         mrcal_lensmodel_num_params(const mrcal_lensmodel_t* lensmodel);

/* reference: mrcal.h:374-375, mrcal.c:361-371 */
int mrcal_num_intrinsics_optimization_params(mrcal_problem_selections_t problem_selections,
                                             const mrcal_lensmodel_t* lensmodel);

/* reference: mrcal.h:388-421, mrcal.c:3450-3735. In place on (Nstate,) */
void mrcal_pack_solver_state_vector  (double* b,
                                      int Ncameras_intrinsics, int Ncameras_extrinsics,
                                      int Nframes,
                                      int Npoints, int Npoints_fixed, int Nobservations_board,
                                      mrcal_problem_selections_t problem_selections,
                                      const mrcal_lensmodel_t* lensmodel);
void mrcal_unpack_solver_state_vector(double* b,
                                      int Ncameras_intrinsics, int Ncameras_extrinsics,
                                      int Nframes,
                                      int Npoints, int Npoints_fixed, int Nobservations_board,
                                      mrcal_problem_selections_t problem_selections,
                                      const mrcal_lensmodel_t* lensmodel);

/* reference: mrcal.h:437-446, mrcal.c:3929-3969 */
bool mrcal_corresponding_icam_extrinsics(int* icam_extrinsics,
                                         int icam_intrinsics,
                                         int Ncameras_intrinsics,
                                         int Ncameras_extrinsics,
                                         int Nobservations_board,
                                         const mrcal_observation_board_t* observations_board,
                                         int Nobservations_point,
                                         const mrcal_observation_point_t* observations_point);

/* reference: mrcal.h:453-521, mrcal.c:6179-6624. The whole solve: dog-leg
   iterations + outlier rejection. In/out arrays are updated in place; new
   outliers are marked by negating observations_board_pool[].z */
mrcal_stats_t
mrcal_optimize( double* b_packed, int buffer_size_b_packed,
                double* x,        int buffer_size_x,
                double*                 intrinsics,
                mrcal_pose_t*           rt_cam_ref,
                mrcal_pose_t*           rt_ref_frame,
                mrcal_point3_t*         points,
                mrcal_calobject_warp_t* calobject_warp,
                int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                int Npoints, int Npoints_fixed,
                const mrcal_observation_board_t* observations_board,
                const mrcal_observation_point_t* observations_point,
                int Nobservations_board,
                int Nobservations_point,
                const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                int Nobservations_point_triangulated,
                mrcal_point3_t* observations_board_pool,
                mrcal_point3_t* observations_point_pool,
                const mrcal_lensmodel_t* lensmodel,
                const int* imagersizes,
                mrcal_problem_selections_t       problem_selections,
                const mrcal_problem_constants_t* problem_constants,
                double calibration_object_spacing,
                int calibration_object_width_n,
                int calibration_object_height_n,
                bool verbose,
                bool check_gradient);

/* Pixel -> observation vector (not normalized). Reference: mrcal.h:177-206,
   mrcal.c:3082-3286. HOST computation, like in the reference: it is the setup
   step that turns triangulated-point pixel observations into the vectors
   mrcal_observation_point_triangulated_t carries (mrcal-pywrap.c:1388-1395) */
bool mrcal_unproject(mrcal_point3_t* out, const mrcal_point2_t* q, int N,
                     const mrcal_lensmodel_t* lensmodel, const double* intrinsics);
/* The batch form ON THE GPU, with the gradients that mrcal.unproject(get_gradients=True)
   reports (mrcal/projections.py:112-395, which derives them from project()'s at the
   solution): dv_dq (N,3,2), dv_dintrinsics (N,3,Nintrinsics), either may be NULL
   (dv_dintrinsics needs dv_dq). Without gradients v is what mrcal_unproject() gives;
   with them it is, like the reference's, the stereographic representative of the
   same direction for the models inverted iteratively. normalize: unit vectors, and
   the gradients of the unit vectors */
bool mrcal_amd_unproject(mrcal_point3_t* v, double* dv_dq, double* dv_dintrinsics,
                         const mrcal_point2_t* q, int N,
                         const mrcal_lensmodel_t* lensmodel, const double* intrinsics, bool normalize);


/* Stand-alone projection of N camera-frame points (reference: mrcal.h:165-174,
   mrcal.c:2867-3069). Host pointers. dq_dp (N,2,3) and dq_dintrinsics
   (N,2,Nintrinsics) may be NULL. Runs the same device functions as the solver's
   kernels, one lane per point */
bool mrcal_project(mrcal_point2_t* q, mrcal_point3_t* dq_dp, double* dq_dintrinsics,
                   const mrcal_point3_t* p, int N,
                   const mrcal_lensmodel_t* lensmodel, const double* intrinsics);

/* reference: mrcal.h:539-609, mrcal.c:5972-6177. One evaluation of the cost
   function: b_packed, x and (if Jt != NULL) the CSR Jacobian: Jt->p
   (int32[Nmeas+1]), Jt->i (int32[Nnz]), Jt->x (double[Nnz]) */
bool mrcal_optimizer_callback(double* b_packed, int buffer_size_b_packed,
                              double* x,        int buffer_size_x,
                              struct cholmod_sparse_struct* Jt,
                              const double*                 intrinsics,
                              const mrcal_pose_t*           rt_cam_ref,
                              const mrcal_pose_t*           rt_ref_frame,
                              const mrcal_point3_t*         points,
                              const mrcal_calobject_warp_t* calobject_warp,
                              int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                              int Npoints, int Npoints_fixed,
                              const mrcal_observation_board_t* observations_board,
                              const mrcal_observation_point_t* observations_point,
                              int Nobservations_board,
                              int Nobservations_point,
                              const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                              int Nobservations_point_triangulated,
                              const mrcal_point3_t* observations_board_pool,
                              const mrcal_point3_t* observations_point_pool,
                              const mrcal_lensmodel_t* lensmodel,
                              const int* imagersizes,
                              mrcal_problem_selections_t       problem_selections,
                              const mrcal_problem_constants_t* problem_constants,
                              double calibration_object_spacing,
                              int calibration_object_width_n,
                              int calibration_object_height_n,
                              bool verbose);

/* reference: mrcal.h:613-669, uncertainty.c:798-1541 (Python: mrcal.drt_cross_reprojection__dbpacked(),
   mrcal-pywrap.c:2012-2110). K_packed = drt_ref_refperturbed/db_packed (icam_intrinsics < 0: "rrp") or
   drt_cam_camperturbed/db_packed for that camera ("ccp"), from the packed Jacobian Jt as
   mrcal_optimizer_callback() fills it and the packed state it was evaluated at. Each Kpacked* is (6, N of that
   block), rows stored densely (stride1 == sizeof(double); strides in bytes, <= 0: contiguous); NULL where the
   block is not in the state. The sums over the rows of J run on the GPU (csrc/uncertainty.hip) */
bool _mrcal_drt_cross_reprojection__dbpacked(double* Kpackede,  int Kpackede_stride0,  int Kpackede_stride1,
                                             double* Kpackedf,  int Kpackedf_stride0,  int Kpackedf_stride1,
                                             double* Kpackedp,  int Kpackedp_stride0,  int Kpackedp_stride1,
                                             double* Kpackedcw, int Kpackedcw_stride0, int Kpackedcw_stride1,
                                             const int icam_intrinsics,
                                             const double* b_packed, int buffer_size_b_packed,
                                             struct cholmod_sparse_struct* Jt,
                                             int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                                             int Npoints, int Npoints_fixed,
                                             int Nobservations_board, int Nobservations_point,
                                             const mrcal_lensmodel_t* lensmodel,
                                             mrcal_problem_selections_t problem_selections,
                                             int calibration_object_width_n, int calibration_object_height_n);

/* reference: mrcal.h:713-853 (layout of the measurement and state vectors),
   mrcal.c:337-735, 3737-3880 */
int mrcal_measurement_index_boards(int i_observation_board,
                                   int Nobservations_board, int Nobservations_point,
                                   int calibration_object_width_n, int calibration_object_height_n);
int mrcal_num_measurements_boards(int Nobservations_board,
                                  int calibration_object_width_n, int calibration_object_height_n);
int mrcal_measurement_index_points(int i_observation_point,
                                   int Nobservations_board, int Nobservations_point,
                                   int calibration_object_width_n, int calibration_object_height_n);
int mrcal_num_measurements_points(int Nobservations_point);
int mrcal_measurement_index_points_triangulated(int i_point_triangulated,
                                                int Nobservations_board, int Nobservations_point,
                                                const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                                                int Nobservations_point_triangulated,
                                                int calibration_object_width_n, int calibration_object_height_n);
int mrcal_num_measurements_points_triangulated(const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                                               int Nobservations_point_triangulated);
int mrcal_num_measurements_points_triangulated_initial_Npoints(const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                                                               int Nobservations_point_triangulated,
                                                               int Npoints);
bool mrcal_decode_observation_indices_points_triangulated(int* iobservation0, int* iobservation1,
                                                          int* iobservation_point0,
                                                          int* Nobservations_this_point,
                                                          int* Nmeasurements_this_point,
                                                          int* ipoint,
                                                          const int imeasurement,
                                                          const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                                                          int Nobservations_point_triangulated);
int mrcal_measurement_index_regularization(const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                                           int Nobservations_point_triangulated,
                                           int calibration_object_width_n, int calibration_object_height_n,
                                           int Ncameras_intrinsics, int Ncameras_extrinsics,
                                           int Nframes,
                                           int Npoints, int Npoints_fixed, int Nobservations_board, int Nobservations_point,
                                           mrcal_problem_selections_t problem_selections,
                                           const mrcal_lensmodel_t* lensmodel);
int mrcal_num_measurements_regularization(int Ncameras_intrinsics, int Ncameras_extrinsics,
                                          int Nframes,
                                          int Npoints, int Npoints_fixed, int Nobservations_board,
                                          mrcal_problem_selections_t problem_selections,
                                          const mrcal_lensmodel_t* lensmodel);
int mrcal_num_measurements(int Nobservations_board, int Nobservations_point,
                           const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                           int Nobservations_point_triangulated,
                           int calibration_object_width_n, int calibration_object_height_n,
                           int Ncameras_intrinsics, int Ncameras_extrinsics,
                           int Nframes,
                           int Npoints, int Npoints_fixed,
                           mrcal_problem_selections_t problem_selections,
                           const mrcal_lensmodel_t* lensmodel);
int mrcal_num_states(int Ncameras_intrinsics, int Ncameras_extrinsics,
                     int Nframes,
                     int Npoints, int Npoints_fixed, int Nobservations_board,
                     mrcal_problem_selections_t problem_selections,
                     const mrcal_lensmodel_t* lensmodel);
int mrcal_state_index_intrinsics(int icam_intrinsics,
                                 int Ncameras_intrinsics, int Ncameras_extrinsics,
                                 int Nframes,
                                 int Npoints, int Npoints_fixed, int Nobservations_board,
                                 mrcal_problem_selections_t problem_selections,
                                 const mrcal_lensmodel_t* lensmodel);
int mrcal_num_states_intrinsics(int Ncameras_intrinsics,
                                mrcal_problem_selections_t problem_selections,
                                const mrcal_lensmodel_t* lensmodel);
int mrcal_state_index_extrinsics(int icam_extrinsics,
                                 int Ncameras_intrinsics, int Ncameras_extrinsics,
                                 int Nframes,
                                 int Npoints, int Npoints_fixed, int Nobservations_board,
                                 mrcal_problem_selections_t problem_selections,
                                 const mrcal_lensmodel_t* lensmodel);
int mrcal_num_states_extrinsics(int Ncameras_extrinsics,
                                mrcal_problem_selections_t problem_selections);
int mrcal_state_index_frames(int iframe,
                             int Ncameras_intrinsics, int Ncameras_extrinsics,
                             int Nframes,
                             int Npoints, int Npoints_fixed, int Nobservations_board,
                             mrcal_problem_selections_t problem_selections,
                             const mrcal_lensmodel_t* lensmodel);
int mrcal_num_states_frames(int Nframes,
                            mrcal_problem_selections_t problem_selections);
int mrcal_state_index_points(int i_point,
                             int Ncameras_intrinsics, int Ncameras_extrinsics,
                             int Nframes,
                             int Npoints, int Npoints_fixed, int Nobservations_board,
                             mrcal_problem_selections_t problem_selections,
                             const mrcal_lensmodel_t* lensmodel);
int mrcal_num_states_points(int Npoints, int Npoints_fixed,
                            mrcal_problem_selections_t problem_selections);
int mrcal_state_index_calobject_warp(int Ncameras_intrinsics, int Ncameras_extrinsics,
                                     int Nframes,
                                     int Npoints, int Npoints_fixed, int Nobservations_board,
                                     mrcal_problem_selections_t problem_selections,
                                     const mrcal_lensmodel_t* lensmodel);
int mrcal_num_states_calobject_warp(mrcal_problem_selections_t problem_selections,
                                    int Nobservations_board);

/* reference: internal.h:99-114, mrcal.c:743-882 */
int _mrcal_num_j_nonzero(int Nobservations_board,
                         int Nobservations_point,
                         const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                         int Nobservations_point_triangulated,
                         int calibration_object_width_n,
                         int calibration_object_height_n,
                         int Ncameras_intrinsics, int Ncameras_extrinsics,
                         int Nframes,
                         int Npoints, int Npoints_fixed,
                         const mrcal_observation_board_t* observations_board,
                         const mrcal_observation_point_t* observations_point,
                         mrcal_problem_selections_t problem_selections,
                         const mrcal_lensmodel_t* lensmodel);

/* .cameramodel files at the C level: the on-disk form of one camera (lens
   model, intrinsics, imager size, pose), a python dict literal. Host code.
   reference: types.h:347-376 (the struct: the intrinsics follow the header, as
   many as mrcal_lensmodel_num_params() says), mrcal.h:858-890 (the functions),
   cameramodel-parser.re:356-790, mrcal.c:6626-6680. Only lensmodel, intrinsics,
   imagersize and extrinsics/rt_cam_ref are read; other keys are skipped. The
   writer prints %.17g (the reference prints %f). */
typedef struct
{
    double            rt_cam_ref[6];
    unsigned int      imagersize[2];
    mrcal_lensmodel_t lensmodel;
    double            intrinsics[0];
} mrcal_cameramodel_VOID_t;
#define mrcal_cameramodel_t mrcal_cameramodel_VOID_t
/* these allocate; release with mrcal_free_cameramodel(). NULL on error. len > 0:
   the string need not be 0-terminated; len <= 0: it is */
mrcal_cameramodel_VOID_t* mrcal_read_cameramodel_string(const char* string, const int len);
mrcal_cameramodel_VOID_t* mrcal_read_cameramodel_file  (const char* filename);
void                      mrcal_free_cameramodel(mrcal_cameramodel_VOID_t** cameramodel);
/* these read into a caller's buffer with room for *Nintrinsics_max intrinsics.
   false on failure; if the buffer was too small, *Nintrinsics_max says what is
   needed, otherwise it comes back <= 0 */
bool mrcal_read_cameramodel_string_into(mrcal_cameramodel_VOID_t* model, int* Nintrinsics_max,
                                        const char* string, const int len);
bool mrcal_read_cameramodel_file_into  (mrcal_cameramodel_VOID_t* model, int* Nintrinsics_max,
                                        const char* filename);
bool mrcal_write_cameramodel_file(const char* filename, const mrcal_cameramodel_VOID_t* cameramodel);

/* ------------------------------------------------------------------------ */
/* RESIDENT TIER                                                             */
/* ------------------------------------------------------------------------ */

/* Returns NULL-terminated static string describing the last error on this
   thread ("" if none) */
const char* mrcal_amd_last_error(void);

/* Number of visible HIP devices; <=0 if there is no usable GPU */
int mrcal_amd_device_count(void);

/* Device and pinned-host buffers the library holds in this process right now, over
   all problems, factorizations and uncertainty contexts: back at its earlier value
   once everything made since has been destroyed (the drop-in entry points tear
   their problem down on a thread of their own, a moment after they return) */
long mrcal_amd_device_buffers_live(void);

typedef struct mrcal_amd_problem mrcal_amd_problem_t;

/* Uploads a whole optimization problem (same arguments as
   mrcal_optimizer_callback(), host pointers) to the current HIP device and
   builds the iteration-invariant structure (state/measurement layout, CSR
   rowptr/colidx) there. Returns NULL on error.

   shard_begin_frame/shard_end_frame select a contiguous range of FRAMES whose
   board observations this problem instance owns (multi-GPU sharding by
   frame, one process per GPU); pass 0,-1 for "everything". All ranks still
   see the full state vector; only the measurements are partitioned.
   is_shard_leader says whether this instance owns the rows that belong to no
   frame (discrete points, triangulated points, regularization). */
mrcal_amd_problem_t*
mrcal_amd_problem_create(const double*                 intrinsics,
                         const mrcal_pose_t*           rt_cam_ref,
                         const mrcal_pose_t*           rt_ref_frame,
                         const mrcal_point3_t*         points,
                         const mrcal_calobject_warp_t* calobject_warp,
                         int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                         int Npoints, int Npoints_fixed,
                         const mrcal_observation_board_t* observations_board,
                         const mrcal_observation_point_t* observations_point,
                         int Nobservations_board,
                         int Nobservations_point,
                         const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                         int Nobservations_point_triangulated,
                         const mrcal_point3_t* observations_board_pool,
                         const mrcal_point3_t* observations_point_pool,
                         const mrcal_lensmodel_t* lensmodel,
                         const int* imagersizes,
                         mrcal_problem_selections_t problem_selections,
                         double calibration_object_spacing,
                         int calibration_object_width_n,
                         int calibration_object_height_n,
                         int shard_begin_frame, int shard_end_frame,
                         bool is_shard_leader);
/* The same with the discrete points and the triangulated points sharded as well: the shard owns
   the points [shard_begin_point, shard_end_point) - their 3x3 blocks, and their observations wherever those sit
   in the caller's array - and the triangulated point SETS [shard_begin_tripoint, shard_end_tripoint) (a set = the
   consecutive observations of one point up to last_in_set; its pairs are its own rows). An end < 0: all of that
   kind with the leader, as mrcal_amd_problem_create() does. The camera block of the state and the regularization
   rows stay with the leader */
mrcal_amd_problem_t*
mrcal_amd_problem_create_sharded(const double*                 intrinsics,
                         const mrcal_pose_t*           rt_cam_ref,
                         const mrcal_pose_t*           rt_ref_frame,
                         const mrcal_point3_t*         points,
                         const mrcal_calobject_warp_t* calobject_warp,
                         int Ncameras_intrinsics, int Ncameras_extrinsics, int Nframes,
                         int Npoints, int Npoints_fixed,
                         const mrcal_observation_board_t* observations_board,
                         const mrcal_observation_point_t* observations_point,
                         int Nobservations_board,
                         int Nobservations_point,
                         const mrcal_observation_point_triangulated_t* observations_point_triangulated,
                         int Nobservations_point_triangulated,
                         const mrcal_point3_t* observations_board_pool,
                         const mrcal_point3_t* observations_point_pool,
                         const mrcal_lensmodel_t* lensmodel,
                         const int* imagersizes,
                         mrcal_problem_selections_t problem_selections,
                         double calibration_object_spacing,
                         int calibration_object_width_n,
                         int calibration_object_height_n,
                         int shard_begin_frame, int shard_end_frame,
                         int shard_begin_point, int shard_end_point,
                         int shard_begin_tripoint, int shard_end_tripoint,
                         bool is_shard_leader);
void mrcal_amd_problem_destroy(mrcal_amd_problem_t* problem);

/* sizes of the LOCAL (this shard's) problem */
int     mrcal_amd_problem_Nstate       (const mrcal_amd_problem_t* problem);
int     mrcal_amd_problem_Nmeasurements(const mrcal_amd_problem_t* problem);
int64_t mrcal_amd_problem_Nnz          (const mrcal_amd_problem_t* problem);
/* Algorithmic HBM bytes of one launch of the board Jacobian kernel on this
   problem: per observation of P corners with k nonzeros per row,
   24 P (read qx,qy,weight) + 16 P (write x) + 16 P k (write J values); where the
   triangulated pairs of a structure-from-motion problem ride in that launch (round 6: a
   problem with boards and pairs whose intrinsics are locked), + per pair 48 (two
   observation vectors) + its record + 8 (x) + 8 per partial written */
int64_t mrcal_amd_problem_jacobian_algorithmic_bytes(const mrcal_amd_problem_t* problem);
/* waits for everything queued on the problem's stream */
bool    mrcal_amd_problem_synchronize  (mrcal_amd_problem_t* problem);

/* Device pointers into the problem's resident buffers (valid until destroy):
   the packed state the next evaluation uses, and the outputs of the last
   evaluation. J is CSR: rowptr int32[Nmeas+1], colidx int32[Nnz], values
   double[Nnz], exactly the arrays mrcal_optimizer_callback() fills */
double*  mrcal_amd_problem_dev_b_packed(mrcal_amd_problem_t* problem);
double*  mrcal_amd_problem_dev_x       (mrcal_amd_problem_t* problem);
int32_t* mrcal_amd_problem_dev_J_rowptr(mrcal_amd_problem_t* problem);
int32_t* mrcal_amd_problem_dev_J_colidx(mrcal_amd_problem_t* problem);
double*  mrcal_amd_problem_dev_J_values(mrcal_amd_problem_t* problem);

/* host <-> device copies of the packed state */
bool mrcal_amd_problem_set_b_packed(mrcal_amd_problem_t* problem, const double* b_packed_host);
bool mrcal_amd_problem_get_b_packed(mrcal_amd_problem_t* problem, double* b_packed_host);
bool mrcal_amd_problem_get_x       (mrcal_amd_problem_t* problem, double* x_host);
/* any of the three may be NULL */
bool mrcal_amd_problem_get_J       (mrcal_amd_problem_t* problem,
                                    int32_t* rowptr_host, int32_t* colidx_host, double* values_host);

/* One evaluation of x (and J if with_jacobian) at the resident packed state.
   Asynchronous on the problem's stream unless sync. This is the Jacobian
   build the roofline is quoted on */
bool mrcal_amd_problem_evaluate(mrcal_amd_problem_t* problem, bool with_jacobian, bool sync);

/* The HIP stream (hipStream_t, as void*) all of this problem's kernels are
   launched on, so that callers can bracket them with their own events */
void* mrcal_amd_problem_stream(mrcal_amd_problem_t* problem);

/* Timing of the most recent evaluation's dominant kernel (the board
   Jacobian build), measured with HIP events on the problem's stream.
   Returns milliseconds, <0 if unavailable */
double mrcal_amd_problem_last_jacobian_kernel_ms(mrcal_amd_problem_t* problem);

/* Records a HIP event pair around every `stride`-th Jacobian-kernel launch from
   now on (up to `capacity` pairs), on the problem's stream; _end() stops, waits
   and reports the number of launches timed and their total/min/max duration
   (ms). This is how the benchmark measures the dominant kernel over its timed
   region. An event pair costs the stream ~11 us (5.6 on each side of the
   kernel), which is why the solver's steps carry none unless asked, and why the
   benchmark asks for a stride. _begin(p, n) == _begin_strided(p, n, 1).
   (mrcal_amd_problem_last_jacobian_kernel_ms() refers to host-driven
   mrcal_amd_problem_evaluate() calls.) */
bool mrcal_amd_problem_jacobian_timing_begin(mrcal_amd_problem_t* problem, int capacity);
bool mrcal_amd_problem_jacobian_timing_begin_strided(mrcal_amd_problem_t* problem, int capacity, int stride);
bool mrcal_amd_problem_jacobian_timing_end(mrcal_amd_problem_t* problem, int* Nlaunches,
                                           double* total_ms, double* min_ms, double* max_ms);
/* Round 5, the splined models with one camera: the camera block's coupled control points in a nested-dissection order
   where the boards leave a strip of the grid worth having - two sides whose panels the big Cholesky
   factors side by side, the strip last. out[9]: the rounds (panels a side) the factorization's launches are provided
   for (0: the dissection is not in use), the largest separator they serve, and the current operating point's plan:
   used or not, the columns of side A, of side B (padded to whole panels of 64), of the separator; what the best strip there would give (side A, side B,
   separator, unpadded). For tests and
   tools; MRCAL_AMD_NO_ND=1 in the environment when the problem is created turns the dissection off */
bool mrcal_amd_problem_dissection(mrcal_amd_problem_t* problem, int* out);

/* ---- multi-GPU: one process per GPU, frames sharded over the ranks ----------
   No counterpart in the reference (it is single-threaded). Every rank creates
   its shard with mrcal_amd_problem_create(shard_begin_frame, shard_end_frame,
   is_shard_leader) from the SAME inputs, attaches a communicator, and calls
   mrcal_amd_problem_solve() / _run_steps() like a single-GPU caller: the
   device-controlled dog-leg step then runs with TWO all-reduces per trial
   step, issued from C++ on the problem's stream (RCCL over xGMI):
       comm 0  [ S (Nc*Nc) | r (Nc) | g_S (Nc) | |x|^2 | status ]   after the local Schur reduction
       comm 1  [ g^T JtJ g | |g_E|^2 | |gn_E|^2 | gn_E . g_E ]       after the local back-substitution
   Rank-local: the frame poses of the shard's frames (state, gradient, steps),
   its rows of x and J. Replicated, and advanced identically by every rank from
   the same sums: the camera block of the state (intrinsics, extrinsics, warp)
   and the trust-region control block. Nothing is read back between trial steps.

   The communicator: rank 0 makes a 128-byte id (mrcal_amd_comm_unique_id),
   any side channel carries it to the other ranks, every rank calls
   mrcal_amd_comm_create(id, rank, world). RCCL is opened at run time */
typedef struct mrcal_amd_comm mrcal_amd_comm_t;
bool              mrcal_amd_comm_unique_id(void* id128);
mrcal_amd_comm_t* mrcal_amd_comm_create(const void* id128, int rank, int world);
/* The same interface over a POSIX shared-memory segment, for the ranks of one
   host: synchronous, staged through host memory, the sum taken in rank order.
   For exercising the sharded solve where RCCL cannot run (two ranks on one
   device); not a transport to measure. name: "/x", unused, the same on every
   rank. A rank that does not arrive within MRCAL_AMD_HOST_COMM_TIMEOUT
   seconds (default 120) makes the collective fail */
mrcal_amd_comm_t* mrcal_amd_comm_create_host(const char* name, int rank, int world);
void              mrcal_amd_comm_destroy(mrcal_amd_comm_t* comm);
int               mrcal_amd_comm_rank (const mrcal_amd_comm_t* comm);
int               mrcal_amd_comm_world(const mrcal_amd_comm_t* comm);
long              mrcal_amd_comm_Ncollectives(const mrcal_amd_comm_t* comm);
long long         mrcal_amd_comm_Ndoubles(const mrcal_amd_comm_t* comm);        /* doubles summed, over all collectives */
int               mrcal_amd_comm_world_observed(const mrcal_amd_comm_t* comm);  /* ncclCommCount(): what the transport itself says */
/* in-place sum over the ranks of n doubles in device memory, queued on the HIP stream */
bool              mrcal_amd_comm_allreduce_sum(mrcal_amd_comm_t* comm, double* buf_dev, int64_t n, void* stream);

/* From now on solve()/run_steps() of this shard run the sharded step over comm
   (not owned; must outlive the problem or be detached with NULL) */
bool  mrcal_amd_problem_attach_comm(mrcal_amd_problem_t* problem, mrcal_amd_comm_t* comm);
/* after a solve: every rank gets the whole state (the frame poses of the
   other ranks' frames) into its resident b_packed. One all-reduce of Nstate doubles */
bool  mrcal_amd_problem_gather_state(mrcal_amd_problem_t* problem);

/* The same step for a driver that brings its OWN collectives (the protocol
   tests: mrcal_amd/parallel.py drives two shards on one device over gloo). Per
   trial step the driver queues, on the problem's stream,
       enqueue(0,0) | all-reduce comm_buffer(0) | enqueue(0,1) | all-reduce comm_buffer(1)
   and never reads anything back in between. initial=1: the evaluation of the
   starting point. enqueue() refuses a problem sharded_reset() has not been called
   on (mrcal_amd_last_error()). snapshot(slot)/wait(slot): a pinned copy
   of the control block, queued after a trial step and waited for a few steps
   later, tells the host when the device has declared the solve finished; wait()
   writes out[4] = { done, error, Nsteps_accepted, Ntrials }. finish() drains the
   stream and makes the final point current; out_i[5] = { Nsteps_accepted,
   Nevaluations, Nfactorizations, Ntrials, error }, out_d[3] = { trust region,
   |x|^2, lambda } */
bool  mrcal_amd_problem_sharded_reset      (mrcal_amd_problem_t* problem, int check_termination, int max_iterations,
                                            double trustregion0);
bool  mrcal_amd_problem_sharded_enqueue    (mrcal_amd_problem_t* problem, int initial, int segment);
void* mrcal_amd_problem_sharded_comm_buffer(mrcal_amd_problem_t* problem, int which, int64_t* Nelements);
bool  mrcal_amd_problem_sharded_snapshot   (mrcal_amd_problem_t* problem, int slot);
bool  mrcal_amd_problem_sharded_wait       (mrcal_amd_problem_t* problem, int slot, int* out);
bool  mrcal_amd_problem_sharded_finish     (mrcal_amd_problem_t* problem, int* out_i, double* out_d);
/* What this shard holds. Writes min(Ninfo, MRCAL_AMD_SHARD_INFO_N) ints and returns how many it knows of (the caller
   says how big its buffer is; the list only ever grows at the end):
     info[0]  Nstate            the full state vector (every shard holds all of it)
     info[1]  S_split           first state index that is NOT one of the leading dense-block variables: in a sharded
                                (frames/points-eliminated) problem the state is [0,S_split) intrinsics + extrinsics,
                                [S_split, S_split+NE) the eliminated variables - frames (6 each), then the variable
                                points (3 each) -, then the board warp (mrcal_amd_problem_partition() has the general form)
     info[2]  NE                number of eliminated variables (all shards' together)
     info[3]  Nc                size of the dense camera block (intrinsics + extrinsics + warp)
     info[4], info[5]  frame_lo, frame_hi     the frames [lo,hi) whose board observations and 6x6 blocks this shard owns
     info[6]  is_leader         this shard owns the camera block of the state, the warp and the regularization rows
     info[7]  Ncorners_local    board corners in this shard's observations
     info[8]  Nframe_blocks     6x6 blocks of the whole problem
     info[9]  Npoint_blocks     3x3 blocks of the whole problem
     info[10], info[11]  point_lo, point_hi   the eliminated BLOCKS [lo,hi), lo >= Nframe_blocks, of the variable points
                                this shard owns (its discrete-point observations and its triangulated pairs) */
#define MRCAL_AMD_SHARD_INFO_N 12
int   mrcal_amd_problem_shard_info(mrcal_amd_problem_t* problem, int* info, int Ninfo);
/* Which pose blocks the problems created from now on eliminate: 0 the library chooses (default: the extrinsics when
   there are at least 4 rt_cam_ref and more extrinsics than frame + point variables, e.g. a moving camera or a big
   stationary rig seen in a handful of frames; the frames and points otherwise), 1 the frames and points, 2 the
   extrinsics where the problem allows it (board rows only, no unity_cam01 row, not splined, not sharded). The results
   of a solve do not depend on it beyond rounding; the block form of mrcal_amd_problem_get_normal_equations() and the
   cost of a step do. Returns the previous setting. (Processes that cannot call it: MRCAL_AMD_ELIMINATE=frames|extrinsics) */
int   mrcal_amd_set_elimination(int policy);
/* Round 6: the solve WITHOUT the Jacobian stream. mrcal_optimize() returns no Jacobian (mrcal.h:453-521) and nothing
   in the device-side dog leg reads the CSR values of J - the per-observation Grams carry the normal equations -, so a
   solve may leave the 16 P k bytes per observation unwritten: the board kernel forms its rows, the
   residuals and the Gram exactly as ever (the same instructions in the same order: x, b_packed, the outlier marks and
   every statistic come out THE SAME BITS) and does not stream the rows to HBM. A product mode; the benchmark's metric -
   a step = one evaluation of x AND J + one solve of the normal equations - is measured with the stream on.
     mrcal_amd_problem_set_jacobian_stream(problem, 0)   _solve() / _run_steps() of this resident problem leave the stream
         out (default 1: on). J is then made on demand: _get_J(), _dev_J_values() and _evaluate(with_jacobian) evaluate
         it at the resident state first. Honoured where the board kernel is the rows' only reader
         (_jacobian_stream_is_optional(): boards under a parametric lens model; the splined models' assembly reads
         the rows back, discrete points and triangulated pairs keep theirs: a few MB)
     mrcal_amd_set_optimize_jacobian_stream(1)   the drop-in mrcal_optimize(), whose problem does not outlive the call,
         streams J all the same (default 0: it does not)
   Both return the previous setting */
/* Hooks for the TESTS (not configuration): force, for the problems prepared after the call, paths a solve takes by
   itself only when a later point outgrows what its first point needed, so that the suite can hold them to the bits of
   the ordinary path. "lchol_likely_panels" = k: k launches of the big camera block's Cholesky are provided one by one,
   the rest goes through lchol_tail_kernel; "nd_rounds" = k: launches for k rounds of the nested dissection whatever
   the plan needs; "lchol_sweep" = 1: the big Cholesky's solve by the backward sweep (the stable fallback the solver
   switches to by itself when a factor's diagonal spans more than 1e10); "lchol_fallback_log10" = k: that threshold as
   10^k. 0: not forced. Returns the previous value,
   -1 for an unknown name. (Round 6: these were environment variables; the library reads five of those now -
   MRCAL_AMD_ELIMINATE, _RCCL, _LIB, _NO_ND, _NO_SPL_COMPACT - and MRCAL_AMD_DEBUG_SOLVER, which only prints) */
int   mrcal_amd_set_test_hook(const char* name, int value);
/* Round 6: the big camera block's solve ends with d = -Y^T z, Y = L^-1 formed explicitly beside the panels: fast, and
   not backward stable - its error grows like n eps max/min of L's diagonal. The factorizations of a dog-leg pass leave
   that ratio behind (_lchol_diag_ratio(): min / max, 1 where no such factorization ran); below 1e-10 (the test hook
   "lchol_fallback_log10" = k: 10^k) the solver warns and switches THIS problem to the backward sweep in groups of panels
   for good (_uses_sweep(): no explicit inverse, no compaction of the camera block; about 100 us a step slower), from the
   next dog-leg pass on */
double mrcal_amd_problem_lchol_diag_ratio(mrcal_amd_problem_t* problem);
int    mrcal_amd_problem_uses_sweep(mrcal_amd_problem_t* problem);
int   mrcal_amd_problem_set_jacobian_stream(mrcal_amd_problem_t* problem, int stream);
int   mrcal_amd_problem_jacobian_stream_is_optional(mrcal_amd_problem_t* problem);
int   mrcal_amd_set_optimize_jacobian_stream(int stream);
/* Which part of the state the solver keeps as the dense block S and which it
   eliminates block by block (E). The state vector is the reference's either way;
     S index s -> state s (s < info[0]) or s + info[1];   E index e -> state info[2] + e
   info[3]: 0 the frames and points are eliminated (stationary cameras), 1 the
   extrinsics are (a moving camera: many rt_cam_ref, few frames; chosen at
   creation, test_calibration_helpers.py:422-493 builds such problems). The
   blocks of mrcal_amd_problem_get_normal_equations() are in these indices */
void  mrcal_amd_problem_partition(mrcal_amd_problem_t* problem, int info[4]);
/* The outlier bits of this problem's (this shard's) triangulated observations after a solve: flags[i] (0/1, at most
   Nflags written) belongs to observations_point_triangulated[*first + i] of the array the problem was created from.
   Returns the number of observations the problem holds. mrcal_optimize() writes them into the caller's array like
   the reference does (mrcal.c:4225, 4375); a sharded solve leaves the gathering to its driver */
int   mrcal_amd_problem_get_triangulated_outliers(mrcal_amd_problem_t* problem, int* flags, int Nflags, int* first);
/* outlier statistics / marking on the local board observations (mrcal.c:3978-4402);
   counts (device int[4]) and sums (device double[1]) are accumulated into */
bool  mrcal_amd_problem_phase_outlier_stats(mrcal_amd_problem_t* problem, int iop, double thresh_sq,
                                            int* counts_dev, double* sums_dev);
bool  mrcal_amd_problem_phase_mark_outliers(mrcal_amd_problem_t* problem, int iop, double thresh_sq, int* counts_dev);
/* which operating point get_b_packed()/get_x()/get_J() read */
void  mrcal_amd_problem_set_current(mrcal_amd_problem_t* problem, int iop);
int   mrcal_amd_problem_current(mrcal_amd_problem_t* problem);

/* The whole solve on a resident problem: dog-leg iterations + outlier
   rejection (if the problem selections ask for it), exactly what
   mrcal_optimize() does between packing and unpacking the state. Returns the
   rms error sqrt(|x|^2/Nmeasurements), <0 on failure. max_iterations<=0: the
   reference's 300. The solution stays resident: read it with
   mrcal_amd_problem_get_b_packed()/get_x() */
double mrcal_amd_problem_solve(mrcal_amd_problem_t* problem, int max_iterations,
                               int* Noutliers_board);

/* Exactly Nsteps dog-leg steps (accepted or rejected) from the current
   operating point, without termination tests or outlier rejection: the unit
   of work the benchmark times. trustregion_inout (may be NULL) carries the
   trust-region radius across calls; <=0 on input means "the default".
   Returns the number of steps taken, <0 on error */
int mrcal_amd_problem_run_steps(mrcal_amd_problem_t* problem, int Nsteps, double* trustregion_inout);

/* Counters of the most recent solve / run_steps. Any pointer may be NULL */
void mrcal_amd_problem_solver_stats(mrcal_amd_problem_t* problem,
                                    int* Niterations, int* Nevaluations, int* Nfactorizations,
                                    int* Noutlier_passes, double* norm2_x, double* lambda, double* seconds);

/* K (6, Nstate) row-major of _mrcal_drt_cross_reprojection__dbpacked() from the Jacobian the problem holds
   (evaluated here at its current state; nothing crosses PCIe but K and one small record per observation).
   Zero outside the extrinsics / frames / points / calobject_warp blocks, like the reference's wrapper leaves it */
bool mrcal_amd_problem_drt_cross_reprojection(mrcal_amd_problem_t* problem, int icam_intrinsics, double* K);

/* Test/diagnostic access. Evaluates at the resident state and copies out the
   normal equations N = JtJ in the solver's block form (see
   csrc/solver_kernels.hip): A (Nc*Nc), Bt (NE*Nc), D (NEb*6*6), g = Jt x
   (Nstate), |x|^2; dims = {Nc, NE, NEb, Nfb, S_split, Nwarp}: S_split as in
   mrcal_amd_problem_partition() - with the frames eliminated it is the number of
   intrinsics + extrinsics variables ("Nie" before round 3); with the extrinsics
   eliminated (moving cameras) it is the number of intrinsics variables, and the
   frames follow in S behind the shift. Any pointer may be NULL */
bool mrcal_amd_problem_get_normal_equations(mrcal_amd_problem_t* problem,
                                            double* A, double* Bt, double* D, double* g,
                                            double* norm2_x, int* dims);
/* d = -(JtJ + lambda I)^-1 Jt x at the resident state, d (Nstate) to the host */
bool mrcal_amd_problem_gauss_newton_step(mrcal_amd_problem_t* problem, double* step);
/* the board observation pool of this shard, with any newly marked outliers */
bool mrcal_amd_problem_get_board_pool(mrcal_amd_problem_t* problem, mrcal_point3_t* pool_local);

/* ---- factorization of JtJ: the CHOLMOD_factorization equivalent -----------
   Reference: the mrcal.CHOLMOD_factorization Python type, mrcal-pywrap.c:111-214
   (constructor from Jt), :425-569 (solve_xt_JtJ_bt), :580-592 (rcond).
   The Jacobian comes as a host CSR matrix (Nmeas x Nstate, int32 offsets, packed
   units), exactly what optimizer_callback() returns. The state partition tells
   the structured solver which variables form the dense shared block (the first
   Nstate_shared_leading: intrinsics and extrinsics; plus the last Nwarp) and
   which are the mutually independent 6x6 frame / 3x3 point blocks in between.
   Pass (Nstate,0,0,0) for a matrix without that structure (dense; small only).
   The shared block must hold at least one variable: Nstate_shared_leading + Nwarp == 0
   is refused (NULL, with a message).
   Returns NULL if JtJ is not positive definite (the reference returns None) */
typedef struct mrcal_amd_factorization mrcal_amd_factorization_t;
mrcal_amd_factorization_t*
mrcal_amd_factorization_create(int Nmeas, int Nstate,
                               const int32_t* rowptr, const int32_t* colidx, const double* values,
                               int Nstate_shared_leading, int Nframe_blocks, int Npoint_blocks, int Nwarp);
/* The same object from a resident problem, at its current state: x, J and the block normal equations by the problem's own
   kernels (no atomics: the same bits every time), copied device to device. What optimizer_callback() returns */
mrcal_amd_factorization_t* mrcal_amd_factorization_create_from_problem(mrcal_amd_problem_t* problem);
/* Why the last _create() / _create_from_problem() of the calling thread returned what it did: 0 a factorization; 1 NULL
   because JtJ is not positive definite (the reference's None, mrcal-pywrap.c:1981-1988); 2 NULL for any other reason
   (no device memory, a shard, a matrix without the declared structure): mrcal_amd_last_error() says which */
int mrcal_amd_factorization_last_status(void);
int    mrcal_amd_factorization_Nmeasurements(const mrcal_amd_factorization_t* f);
void   mrcal_amd_factorization_destroy(mrcal_amd_factorization_t* f);
int    mrcal_amd_factorization_Nstate (const mrcal_amd_factorization_t* f);
/* xt[i,:] = (JtJ)^-1 bt[i,:]; host, C-contiguous (Nrhs,Nstate) */
bool   mrcal_amd_factorization_solve  (mrcal_amd_factorization_t* f, const double* bt, int Nrhs, double* xt);
/* The other systems of cholmod_solve2() (mrcal-pywrap.c:467-493), sys = CHOLMOD's codes:
   0 A, 1 LDLt, 2 LD, 3 DLt, 4 L, 5 Lt, 6 D, 7 P, 8 Pt. The factorization kept here is
       L L^T = P (JtJ) P^T      (an LL^T factorization: D = I, so LD == L, DLt == Lt)
   with P the ordering [ frame blocks | point blocks | intrinsics, extrinsics | warp ]: the
   eliminated blocks first. As with CHOLMOD, the vectors of the L/D systems are in the
   order of P; "P" takes a vector there (x = P b), "Pt" back. mrcal's projection
   uncertainty does  A1 = solve(b,'P'); A2 = solve(A1,'L'); A3 = solve(A2,'D');
   Var = A2 A3^T  (mrcal/model_analysis.py:837-843): the same three calls work here */
bool   mrcal_amd_factorization_solve_sys(mrcal_amd_factorization_t* f, int sys, const double* bt, int Nrhs, double* xt);
/* The consumers of J that go with it (mrcal-genpywrap.py:477-731), on the J the
   factorization was made from, which is resident on the device:
   y (Nstate) = Jt x (Nmeas) ; out (Nx*Nx) = A Jt J At over the leading rows of J, A (Nx*Nstate), Nx <= 8 */
bool   mrcal_amd_factorization_Jt_x     (mrcal_amd_factorization_t* f, const double* x, double* y);
bool   mrcal_amd_factorization_A_Jt_J_At(mrcal_amd_factorization_t* f, const double* A, int Nx, int Nleading_rows_J, double* out);
/* the same for a CSR matrix in host memory (the reference's signatures: mrcal._mrcal_npsp._Jt_x, _A_Jt_J_At) */
bool   mrcal_amd_csr_Jt_x     (int Nrows, int Ncols, const int32_t* Jp, const int32_t* Ji, const double* Jx,
                               const double* x, double* y);
bool   mrcal_amd_csr_A_Jt_J_At(int Nrows, int Ncols, const int32_t* Jp, const int32_t* Ji, const double* Jx,
                               const double* A, int Nx, int Nleading_rows_J, double* out);
/* (min diag L / max diag L)^2, like cholmod_rcond() */
double mrcal_amd_factorization_rcond  (mrcal_amd_factorization_t* f);

/* ---- projection uncertainty: mrcal.projection_uncertainty() ---------------
   Reference: mrcal/model_analysis.py:1192-1517 (projection_uncertainty), :560-870
   (_propagate_calibration_uncertainty), :491-557 (the estimate of the observed
   pixel uncertainty). The cross-reprojection methods only; "mean-pcam" is not
   provided.
   _create() computes, at the problem's current state, the k x k matrix C with
       Var(q) = sigma^2 G(p) C G(p)^T
   (G: the 2 x k gradient of a projection with respect to this camera's optimized
   intrinsics, for rrp its extrinsics, and the 6 rows of
   mrcal_amd_problem_drt_cross_reprojection()), all of it on the device: x and J at
   the state, K, the factorization of J*^T J*, k right-hand sides solved there, C.
   Only K (6 x Nstate) and a few small records cross PCIe. The problem may be
   changed or destroyed afterwards: the context keeps C, the camera's intrinsics and
   pose, and sigma.
   observed_pixel_uncertainty <= 0: sigma is estimated from the board and point
   measurements at the state (RMS / sqrt(1 - Nstate/Nmeasurements)).
   NULL on failure (mrcal_amd_last_error(): the reference's messages: triangulated
   points present, rrp on a moving camera, a singular J^T J, a shard, ...).
   _evaluate(): p_cam (N,3) host, out (N,4) for the covariance (row-major 2x2),
   (N,) for the two standard deviations. Results are the same bits on every call */
#define MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_CCP     0
#define MRCAL_AMD_UNCERTAINTY_CROSS_REPROJECTION_RRP_JFP 1
#define MRCAL_AMD_UNCERTAINTY_COVARIANCE                 0
#define MRCAL_AMD_UNCERTAINTY_WORSTDIRECTION_STDEV       1
#define MRCAL_AMD_UNCERTAINTY_RMS_STDEV                  2
typedef struct mrcal_amd_uncertainty mrcal_amd_uncertainty_t;
mrcal_amd_uncertainty_t* mrcal_amd_uncertainty_create(mrcal_amd_problem_t* problem, int icam_intrinsics, int method,
                                                      double observed_pixel_uncertainty);
bool   mrcal_amd_uncertainty_evaluate(mrcal_amd_uncertainty_t* u, const double* p_cam, int N, bool atinfinity, int what,
                                      double* out);
/* the sigma in use: the caller's, or the estimate */
double mrcal_amd_uncertainty_observed_pixel_uncertainty(const mrcal_amd_uncertainty_t* u);
void   mrcal_amd_uncertainty_destroy(mrcal_amd_uncertainty_t* u);

/* ---- projection differences: mrcal.projection_diff() ----------------------
   Reference: mrcal/model_analysis.py:27-395 (implied_Rt10__from_unprojections), :1520-1928 (projection_diff).
   The implied transformation: the rt10 (r at infinity; t is then 0) that minimises
       F = 1/2 sum C^2 rho(x_i^2/C^2),  x_i = 2 (1 - v1_i . p/|p|) w_i,  p = R(r) p0_i + t
   (C = (5 deg)^2, rho = scipy's 'huber': the reference's cost) over the points with |q0 - focus_center| <
   focus_radius, by damped Gauss-Newton from rt = 0 in ONE launch of one workgroup (csrc/projection_diff.hip): the
   same bits on every call. Non-finite weights count as 0, a non-finite component of p0 or v1 zeroes its point's
   weight, and so does a p0 or a v1 that is the zero vector (a failed unprojection, normalized: a constant in the
   reference's cost, or 0/0 at the start). q0 (N,2), p0 (M,N,3), v1 (N,3) unit vectors, weights (M,N) or NULL: host pointers.
   status: 0 converged; 1 the bound on cost evaluations (400) was reached; 3 no descent step was found (both leave the
   best rt seen, and are not errors); 2 fewer than 3 points in the focus region: false, "Focus region contained too
   few points". cost, Nevaluations, Nused, status may be NULL */
#define MRCAL_AMD_IMPLIED_RT10_CONVERGED      0
#define MRCAL_AMD_IMPLIED_RT10_BOUND          1
#define MRCAL_AMD_IMPLIED_RT10_TOO_FEW_POINTS 2
#define MRCAL_AMD_IMPLIED_RT10_STALLED        3
bool mrcal_amd_implied_rt10(double* rt10 /*6*/, double* cost, int* Nevaluations, int* Nused, int* status,
                            const double* q0 /*N,2*/, const double* p0 /*M,N,3*/, const double* v1 /*N,3*/,
                            const double* weights /*M,N or NULL*/, int M, int N, bool atinfinity,
                            const double focus_center[2], double focus_radius);
/* The resident form. _create(): the pixels q0 (N,2) unprojected through every one of the Nmodels >= 2 models
   (intrinsics[i]: that model's parameters; a CAHVORE model must have E = 0), the unit vectors kept on the device.
   _evaluate(), for Ndistances distances (at infinity: one distance of 1), model 0 against each of the others:
     fit: the implied transformations, all Nmodels-1 in one launch, from p0 = v[0] d over all the distances;
          uncertainties (Nmodels contexts, or NULL: equal weights) give the weights 1/(u_0 u_i)^2 of the
          worst-direction standard deviations at v[i] d. Rt10 (Nmodels-1,4,3) comes back as the device used it, with
          rt10 (Nmodels-1,6), cost, Nevaluations, Nused, status (Nmodels-1 each; any may be NULL)
     otherwise Rt10 is the caller's
     diff (Nmodels-1,Ndistances,N,2; may be NULL) = project_i(Rt10_i (v[0] d)) - q0, difflen (Ndistances,N) its
     length: the root-mean-square over the models when there are more than two.
   The vectors, the weights and the pixels stay on the device between the stages. _time_fit(on): bracket the fit's launch with events from now on; returns the last one's ms (< 0: none) */
typedef struct mrcal_amd_projection_diff mrcal_amd_projection_diff_t;
mrcal_amd_projection_diff_t*
mrcal_amd_projection_diff_create(int Nmodels, const mrcal_lensmodel_t* lensmodels, const double* const* intrinsics,
                                 const double* q0, int N);
bool   mrcal_amd_projection_diff_evaluate(mrcal_amd_projection_diff_t* pd,
                                          const double* distances, int Ndistances, bool atinfinity,
                                          mrcal_amd_uncertainty_t* const* uncertainties,
                                          bool fit, const double focus_center[2], double focus_radius,
                                          double* Rt10, double* rt10, double* cost, int* Nevaluations, int* Nused, int* status,
                                          double* difflen, double* diff);
double mrcal_amd_projection_diff_time_fit(mrcal_amd_projection_diff_t* pd, bool on);
void   mrcal_amd_projection_diff_destroy(mrcal_amd_projection_diff_t* pd);

/* ---- lens-model fit: mrcal-convert-lensmodel --sampled ----------------------
   Reference: mrcal-convert-lensmodel:725-792 (the sampled problem), mrcal.c:4900-5176 (a point observation's rows),
   :5655-5901 (the regularization rows), :6607-6612 (the rms).
   N points p_i (N,3), fixed, in the from-camera's coordinates (do_optimize_frames = false), observed at q_i (N,2) with
   weights w_i (N; NULL: all 1). The unknowns b are the intrinsics of ONE parametric lens model - all of them, or
   without the core (fx,fy,cx,cy) when optimize_core is false: they then start at index 4 - and, with
   optimize_extrinsics, the pose rt_cam_ref (T below; the identity otherwise). What is minimised is the reference's
       F(b) = x.x,   x = ( w_i (project(T p_i) - q_i)   two rows a point;
                           s_j k_j                       a row each distortion term k_j: s_j = 0.1, but 0.5 for the
                                                         three terms of the denominator of OPENCV8 and OPENCV12;
                           s_c (c_xy - (size_xy - 1)/2)  two rows, s_c = 1/width for BOTH, only with optimize_core )
   the last two kinds only with apply_regularization (mrcal.optimize() has it on by default); no unity_cam01 row. A
   point with w_i <= 0 or with a non-finite w_i, p_i or q_i takes no part: its two rows are 0, as the reference's
   are for an outlier, and they still count in Nmeasurements = 2 N + the regularization rows. The reference's scales
   are constants here: mrcal.c computes the number of non-regularization measurements beside them (:5697) but the
   scales do not use it, and this version of the reference gives a point observation no range row (:4990-5003).
       rms_reproj_error__pixels = sqrt(F/Nmeasurements)      the reference's definition, regularization rows and all
   The iteration, from a start b: damped Gauss-Newton on H = J^T J, g = J^T x,
       (H + lambda diag(H)) d = -g,   lambda = 1 at the start of a stage
   (a variable nothing depends on stays put). The trial b + d is kept only if F does not rise; lambda then follows
   Nielsen's rule from the gain ratio, and is multiplied by 2, 4, 8 ... after rejections in a row. A stage ends
     0 converged   F <= sum w_i^2 (64 eps)^2 (|q_i|^2 + 1): a perfect fit as far as doubles can tell; or g = 0; or a step
                   with lambda <= 1 that was kept gained, or one about to be tried is promised by the quadratic
                   model, no more than 1e-12 F
     1 bound       max_evaluations evaluations of F were made in this stage, the one at its start included
                   (0: the default, 200). The best point seen is returned; with max_evaluations = 1 that is the start
     2 too few     fewer pixel rows of points that take part than unknowns. The cost is NaN
     3 stalled     lambda passed 1e10 without a step that lowers F, or F or g is not finite at the start (a NaN in
                   a seed): no descent to be had. The best point seen is returned
   A trial: stage 1 fits the intrinsics alone with T the identity; stage 2, with optimize_extrinsics, continues from
   the result of stage 1 with the six pose variables added, started at rt_seed (NULL: 0) - the reference's two calls
   of mrcal.optimize(). What is reported is the last stage's state and status, and the evaluations of both stages.
   A stage with no unknowns (no distortion terms, no core) is skipped.
   All Ntrials trials run in ONE launch, a workgroup each (csrc/lensfit.hip), from intrinsics_seed (Ntrials,
   Nintrinsics) and rt_seed (Ntrials,6): every sum in a fixed order, so a trial has the same bits on every call and
   whatever the other trials of the call. Results per trial: intrinsics (Ntrials,Nintrinsics), rt (Ntrials,6), cost,
   rms, Nevaluations, status (Ntrials each; any may be NULL). *ibest: the trial with the lowest rms among those that
   are not status 2 and have a finite rms, the first of equals; -1 if there is none.
   false (mrcal_amd_last_error()): a splined model (it is fitted by mrcal_optimize()), an unknown model, fewer pixel
   rows than unknowns, nothing to fit, sizes out of range. Host pointers throughout; the object keeps its device
   buffers and stream between calls. _last_ms(): the device time of the last fit's launch, from events (< 0: none) */
#define MRCAL_AMD_LENSFIT_CONVERGED      0
#define MRCAL_AMD_LENSFIT_BOUND          1
#define MRCAL_AMD_LENSFIT_TOO_FEW_POINTS 2
#define MRCAL_AMD_LENSFIT_STALLED        3
typedef struct mrcal_amd_lensfit mrcal_amd_lensfit_t;
mrcal_amd_lensfit_t* mrcal_amd_lensfit_create(void);
bool   mrcal_amd_lensfit_fit(mrcal_amd_lensfit_t* lf,
                             const double* p /*N,3*/, const double* q /*N,2*/, const double* w /*N or NULL*/, int N,
                             const mrcal_lensmodel_t* lensmodel, const int imagersize[2],
                             const double* intrinsics_seed /*Ntrials,Nintrinsics*/, const double* rt_seed /*Ntrials,6 or NULL*/,
                             int Ntrials,
                             bool optimize_core, bool optimize_extrinsics, bool apply_regularization, int max_evaluations,
                             double* intrinsics, double* rt, double* cost, double* rms, int* Nevaluations, int* status,
                             int* ibest);
double mrcal_amd_lensfit_last_ms(const mrcal_amd_lensfit_t* lf);
/* What _fit() would decide for these arguments, without touching a device (csrc/lensfit_plan.hpp): plan_out[14] =
   PROJ, NDIST (the kernel's instantiation: the row of the lens table), Nintrinsics, the first intrinsic that is an
   unknown (0 or 4), stages, the unknowns of stage 1 and of stage 2 (0: no such stage), the sums a workgroup keeps,
   threads, doubles in a staged row, rows in a chunk, LDS bytes, Nmeasurements, the LDS bytes a workgroup may take.
   false: _fit() would refuse, mrcal_amd_last_error() says why */
#define MRCAL_AMD_LENSFIT_PLAN_N 14
bool   mrcal_amd_lensfit_plan(int* plan_out, const mrcal_lensmodel_t* lensmodel, int N, int Ntrials, const int imagersize[2],
                              bool optimize_core, bool optimize_extrinsics, bool apply_regularization);
void   mrcal_amd_lensfit_destroy(mrcal_amd_lensfit_t* lf);

/* ---- triangulation: mrcal.triangulate_*() ----------------------------------
   Reference: triangulation.h / triangulation.cc (mrcal_triangulate_geometric, _lindstrom, _leecivera_l1, _linf,
   _mid2, _wmid2), broadcast by mrcal/triangulation.py. The batch forms ON THE GPU, one lane per pair
   (csrc/triangulation.hip over csrc/triangulation_math.hpp): host arrays in and out.
     v0, v1 (N,3): the two observation vectors, not necessarily normalized, BOTH in camera-0 coordinates;
     t01 (N,3):    the origin of camera 1 in camera-0 coordinates;
     p (N,3):      the point in camera-0 coordinates; (0,0,0) where the rays are parallel or divergent;
     dp_dv0, dp_dv1, dp_dt01 (N,3,3): the gradients; each may be NULL. All zero where p is (0,0,0).
   _lindstrom() differs as the reference's does: v0_local, v1_local are in their OWN cameras' coordinates, the pose
   is the whole Rt01 (N,4,3), and its gradient dp_dRt01 is (N,3,4,3).
   p has the same bits with and without gradients, and on every call */
bool mrcal_amd_triangulate_geometric      (int N, const double* v0, const double* v1, const double* t01,
                                           double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01);
bool mrcal_amd_triangulate_lindstrom      (int N, const double* v0_local, const double* v1_local, const double* Rt01,
                                           double* p, double* dp_dv0, double* dp_dv1, double* dp_dRt01);
bool mrcal_amd_triangulate_leecivera_l1   (int N, const double* v0, const double* v1, const double* t01,
                                           double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01);
bool mrcal_amd_triangulate_leecivera_linf (int N, const double* v0, const double* v1, const double* t01,
                                           double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01);
bool mrcal_amd_triangulate_leecivera_mid2 (int N, const double* v0, const double* v1, const double* t01,
                                           double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01);
bool mrcal_amd_triangulate_leecivera_wmid2(int N, const double* v0, const double* v1, const double* t01,
                                           double* p, double* dp_dv0, double* dp_dv1, double* dp_dt01);

/* ---- mrcal.triangulate(): pixel pairs -> points, with the noise propagated ----
   Reference: mrcal/triangulation.py:1090-2018 (triangulate(), _triangulation_uncertainty_internal(),
   _compute_Var_q_triangulation()), mrcal/model_analysis.py:560-870 (_propagate_calibration_uncertainty()).
   The resident form. _create(): a table of cameras, each with its lens model, intrinsics and rt_cam_ref; with a
   problem (the calibration all the cameras came out of, at its solved state) also icam_intrinsics and
   icam_extrinsics (< 0: the camera at the reference) in it, and then every camera has the problem's lens model. The
   factorization of J*^T J*, the regularization rows of J, the frames and the estimate of the observed pixel
   uncertainty are made here, once; the problem may be changed or destroyed afterwards. problem == NULL: a context
   that cannot propagate calibration-time noise. A CAHVORE camera must have E = 0.
   _evaluate(): q (N,2,2) pixels, icam (N,2) the two cameras of each pair in the table, method one of
   MRCAL_AMD_TRIANGULATE_*; all host arrays.
     p (N,3):                 the points in the coordinates of each pair's first camera; (0,0,0) for divergent rays
     q_observation_stdev > 0: Var_p_observation (N,3,3) = dp/dq Var_q dp/dq^T, Var_q the 4x4 with
                              q_observation_stdev^2 on the diagonal and (q_observation_stdev
                              q_observation_stdev_correlation)^2 between q0x,q1x and between q0y,q1y. 0: not computed
     q_calibration_stdev:     0: not computed. > 0: the calibration-time pixel noise; < 0: the estimate is used.
                              Var_p_calibration (3N,3N), with the cross terms between the pairs:
                              sigma^2 F (J*^T J*)^-1 J*[obs]^T J*[obs] (J*^T J*)^-1 F^T, F = dp/db_packed, with
                              stabilize_coords in the coordinates of the first camera's housing
   MRCAL_AMD_TRIANGULATE_LINDSTROM only without noise. Nothing uses floating-point atomics: the same bits on every
   call. NULL / false on failure (mrcal_amd_last_error(): the reference's messages) */
#define MRCAL_AMD_TRIANGULATE_GEOMETRIC       0
#define MRCAL_AMD_TRIANGULATE_LINDSTROM       1
#define MRCAL_AMD_TRIANGULATE_LEECIVERA_L1    2
#define MRCAL_AMD_TRIANGULATE_LEECIVERA_LINF  3
#define MRCAL_AMD_TRIANGULATE_LEECIVERA_MID2  4
#define MRCAL_AMD_TRIANGULATE_LEECIVERA_WMID2 5
typedef struct
{
    mrcal_lensmodel_t lensmodel;
    const double*     intrinsics;       /* the lens model's number of parameters */
    double            rt_cam_ref[6];
    int               icam_intrinsics;  /* in the problem; not read without one */
    int               icam_extrinsics;  /* in the problem; < 0: at the reference */
} mrcal_amd_triangulation_camera_t;
typedef struct mrcal_amd_triangulation mrcal_amd_triangulation_t;
mrcal_amd_triangulation_t*
mrcal_amd_triangulation_create(mrcal_amd_problem_t* problem, int Ncameras, const mrcal_amd_triangulation_camera_t* cameras);
bool   mrcal_amd_triangulation_evaluate(mrcal_amd_triangulation_t* t, int N, const double* q, const int* icam, int method,
                                        double q_calibration_stdev, double q_observation_stdev,
                                        double q_observation_stdev_correlation, bool stabilize_coords,
                                        double* p, double* Var_p_observation, double* Var_p_calibration);
/* the estimate of the calibration-time pixel noise; < 0: there is none (no problem, or no observations in it) */
double mrcal_amd_triangulation_observed_pixel_uncertainty(const mrcal_amd_triangulation_t* t);
void   mrcal_amd_triangulation_destroy(mrcal_amd_triangulation_t* t);

/* ---- stereo rectification and image reprojection ---------------------------
   Reference: stereo.h / stereo.c (the prototypes below are the reference's), mrcal/stereo.py,
   mrcal/image_transforms.py. The geometry (mrcal_rectified_resolution(), mrcal_rectified_system2()) is host code and
   needs no GPU: csrc/stereo_geometry.cpp. The maps, the remap and the ranges are kernels: csrc/rectification.hip.
   Host arrays in and out. Only MRCAL_LENSMODEL_LATLON and MRCAL_LENSMODEL_PINHOLE rectify */
bool mrcal_rectified_resolution(/* in, out. > 0: used as given; < 0: autodetected and scaled */
                                double* pixels_per_deg_az, double* pixels_per_deg_el,
                                const mrcal_lensmodel_t* lensmodel, const double* intrinsics,
                                const mrcal_point2_t* azel_fov_deg, const mrcal_point2_t* azel0_deg,
                                const double* R_cam0_rect0, const mrcal_lensmodel_type_t rectification_model_type);
bool mrcal_rectified_system2(unsigned int* imagersize_rectified, double* fxycxy_rectified, double* rt_rect0_ref,
                             double* baseline,
                             double* pixels_per_deg_az, double* pixels_per_deg_el,
                             mrcal_point2_t* azel_fov_deg, mrcal_point2_t* azel0_deg,
                             const double az_edge_margin_deg,
                             const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0,
                             const double* rt_cam0_ref, const double* rt_cam1_ref,
                             const mrcal_lensmodel_type_t rectification_model_type,
                             bool az0_deg_autodetect, bool el0_deg_autodetect,
                             bool az_fov_deg_autodetect, bool el_fov_deg_autodetect);
/* az_edge_margin_deg = 10 */
bool mrcal_rectified_system(unsigned int* imagersize_rectified, double* fxycxy_rectified, double* rt_rect0_ref,
                            double* baseline,
                            double* pixels_per_deg_az, double* pixels_per_deg_el,
                            mrcal_point2_t* azel_fov_deg, mrcal_point2_t* azel0_deg,
                            const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0,
                            const double* rt_cam0_ref, const double* rt_cam1_ref,
                            const mrcal_lensmodel_type_t rectification_model_type,
                            bool az0_deg_autodetect, bool el0_deg_autodetect,
                            bool az_fov_deg_autodetect, bool el_fov_deg_autodetect);
/* rectification_maps: float32 (2, Nel, Naz, 2): where in each camera's image every rectified pixel is looked up */
bool mrcal_rectification_maps(float* rectification_maps,
                              const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0, const double* r_cam0_ref,
                              const mrcal_lensmodel_t* lensmodel1, const double* intrinsics1, const double* r_cam1_ref,
                              const mrcal_lensmodel_type_t rectification_model_type,
                              const double* fxycxy_rectified, const unsigned int* imagersize_rectified,
                              const double* r_rect0_ref);
/* reference: image.h. stride in bytes */
typedef struct { union { struct { int width, height; }; struct { int w, h; }; struct { int cols, rows; }; };
                 int stride; uint16_t* data; } mrcal_image_uint16_t;
typedef struct { union { struct { int width, height; }; struct { int w, h; }; struct { int cols, rows; }; };
                 int stride; double*   data; } mrcal_image_double_t;
/* range = 0 where the disparity is <= 0, < min, > max, or the range is not finite */
bool mrcal_stereo_range_sparse(double* range, const double* disparity, const mrcal_point2_t* qrect0, const int N,
                               const double disparity_min, const double disparity_max,
                               const mrcal_lensmodel_type_t rectification_model_type,
                               const double* fxycxy_rectified, const double baseline);
bool mrcal_stereo_range_dense(mrcal_image_double_t* range, const mrcal_image_uint16_t* disparity_scaled,
                              const uint16_t disparity_scale,
                              const uint16_t disparity_scaled_min, const uint16_t disparity_scaled_max,
                              const mrcal_lensmodel_type_t rectification_model_type,
                              const double* fxycxy_rectified, const double baseline);
/* mrcal_stereo_range_sparse() that also writes p (N,3) = range unproject(qrect0)/|unproject(qrect0)|, the points in
   rectified camera-0 coordinates: mrcal.stereo_unproject(). range or p may be NULL */
bool mrcal_amd_stereo_range_sparse(double* range, double* p, const double* disparity, const mrcal_point2_t* qrect0,
                                   const int N, const double disparity_min, const double disparity_max,
                                   const mrcal_lensmodel_type_t rectification_model_type,
                                   const double* fxycxy_rectified, const double baseline);

/* mrcal.image_transformation_map(): mapxy float32 (H_to, W_to, 2). Per pixel of the TO imager: v = unproject_to(pixel);
   p = A (v, or with distance > 0: v/|v| distance) + t; mapxy = project_from(p). A (3x3) and t (3; NULL: 0) are the
   caller's: a rotation R_from_to; R_from_to and t_from_to with a distance; the inverse homography inv(d R_to_from +
   t_to_from n^T) for a plane. region: a closed contour (Nregion,2) in the FROM imager or NULL; pixels that land
   outside it are -1 (at most 2048 vertices). The same bits on every call */
bool mrcal_amd_image_transformation_map(float* mapxy,
                                        const mrcal_lensmodel_t* lensmodel_from, const double* intrinsics_from,
                                        const mrcal_lensmodel_t* lensmodel_to,   const double* intrinsics_to,
                                        const unsigned int* imagersize_to,
                                        const double* A, const double* t, double distance,
                                        const double* region, int Nregion);
/* mrcal.transform_image(): out[i] = image(mapxy[i]). Exact bilinear interpolation in float32 (cv2.remap()'s 1/32-pixel
   fixed point is NOT imitated), or the nearest pixel (halves to even).
   dtype: MRCAL_AMD_IMAGE_*; channels: 1 or 3, interleaved; every array dense.
   MRCAL_AMD_BORDER_CONSTANT:    a neighbour outside the image is border_value[channel]; a non-finite map entry gives it
   MRCAL_AMD_BORDER_TRANSPARENT: a pixel with any neighbour outside, or a non-finite map entry, keeps what out had */
#define MRCAL_AMD_IMAGE_UINT8   0
#define MRCAL_AMD_IMAGE_UINT16  1
#define MRCAL_AMD_IMAGE_FLOAT   2
#define MRCAL_AMD_INTER_NEAREST 0
#define MRCAL_AMD_INTER_LINEAR  1
#define MRCAL_AMD_BORDER_CONSTANT    0
#define MRCAL_AMD_BORDER_TRANSPARENT 5
bool mrcal_amd_transform_image(void* out, const void* image, int width, int height, int channels, int dtype,
                               const float* mapxy, int width_out, int height_out,
                               int interpolation, int border_mode, const double* border_value /*channels*/);
/* The resident form: both rectification maps made once and kept on the device.
   _maps():    mrcal_rectification_maps()'s array, the same bits
   _rectify(): the two images (width0 x height0, width1 x height1) remapped to out0, out1 (Naz x Nel); the maps do
               not leave the device
   _range():   mrcal_stereo_range_dense() of a dense (Nel,Naz) disparity, on the device */
typedef struct mrcal_amd_rectification mrcal_amd_rectification_t;
mrcal_amd_rectification_t*
mrcal_amd_rectification_create(const mrcal_lensmodel_t* lensmodel0, const double* intrinsics0, const double* r_cam0_ref,
                               const mrcal_lensmodel_t* lensmodel1, const double* intrinsics1, const double* r_cam1_ref,
                               const mrcal_lensmodel_type_t rectification_model_type,
                               const double* fxycxy_rectified, const unsigned int* imagersize_rectified,
                               const double* r_rect0_ref, double baseline);
bool mrcal_amd_rectification_maps(mrcal_amd_rectification_t* r, float* rectification_maps);
bool mrcal_amd_rectification_rectify(mrcal_amd_rectification_t* r, void* out0, void* out1,
                                     const void* image0, int width0, int height0,
                                     const void* image1, int width1, int height1, int channels, int dtype,
                                     int interpolation, int border_mode, const double* border_value);
bool mrcal_amd_rectification_range(mrcal_amd_rectification_t* r, double* range, const uint16_t* disparity_scaled,
                                   uint16_t disparity_scale, uint16_t disparity_scaled_min, uint16_t disparity_scaled_max);
void mrcal_amd_rectification_destroy(mrcal_amd_rectification_t* r);

/* ---- match_feature: template matching between two images --------------------
   mrcal.match_feature() (mrcal/stereo.py), which hands the correlation to cv2.matchTemplate(); here it is
   csrc/match_feature.hip, planned on the host by csrc/match_plan.hpp. Both images (grayscale, dense, the same
   MRCAL_AMD_IMAGE_* dtype) are uploaded once by _create(); _match() then finds N features of image0 in image1.

   A feature: q1e (its estimate in image1), H01 (3x3, row-major: image1 pixels -> image0 pixels; the caller inverts its
   H10, the library inverts nothing), the template's size (tw,th) and the search radius r, the same for all N:
     1. tmin = rint(q1e - ((tw,th) - 1)/2), tmax = tmin + (tw,th) - 1: both inside image1, or the status is 3
     2. the template = image0 remapped (bilinear, 0 outside, integers rounded to nearest: mrcal_amd_transform_image())
        through H01 applied to the integer pixels tmin..tmax, in double, rounded to float32; the four corners of that
        map inside image0, or the status is 4
     3. the cut of image1 that is searched: qmin = max(tmin - r, 0) .. qmax = min(tmin + r + (tw,th) - 1, size - 1);
        the match surface has (qmax - qmin + 1) - (tw,th) + 1 entries each way
     4. per entry, over its window of the cut: IT = sum I T, SI = sum I, SI2 = sum I^2; ST, ST2 of the template; N = tw th.
        Integer images: exact integers (uint8 in 32 bits: a template of more than 66051 pixels is refused; uint16 in 64
        bits). float32: summed in double in a fixed order
     5. the method's formula in double, rounded to float32:
          SQDIFF  SI2 - 2 IT + ST2       SQDIFF_NORMED  that / sqrt(SI2 ST2)
          CCORR   IT                     CCORR_NORMED   IT / sqrt(SI2 ST2)
          CCOEFF  IT - SI ST/N           CCOEFF_NORMED  that / sqrt(max(SI2 - SI SI/N, 0) max(ST2 - ST ST/N, 0))
        a denominator that is not > 0: 0 (SQDIFF_NORMED: 1)
     6. the optimum: the minimum (SQDIFF, SQDIFF_NORMED) or the maximum; of equal ones the first in row-major order.
        On the edge of the surface: status 1
     7. the least-squares quadric through the 3x3 entries around it, its stationary point xy (det == 0 or a result
        that is not finite: status 2); q1 = optimum + xy + qmin + q1e - tmin
   status: 0 ok; 1 the optimum is on the edge; 2 the subpixel fit is degenerate; 3 the template is outside image1;
   4 outside image0. A row that is not 0 has NaN in q1, optimum_subpixel_at and optimum_subpixel. _match() returns
   false only for what is wrong whatever the data (sizes that are refused, a device error), never for a status.
   qmin (N,2) and output_size (N,2: width, height; 0 for status 3 and 4) are what _matchoutput() and the caller need
   to read a surface. _matchoutput(i) and _template(i) copy out what the last _match() left on the device: the
   surface of feature i (float32, output_size[i] entries) and its template (tw x th pixels of the images' dtype).
   No atomics: the same bits on every call */
#define MRCAL_AMD_TM_SQDIFF        0
#define MRCAL_AMD_TM_SQDIFF_NORMED 1
#define MRCAL_AMD_TM_CCORR         2
#define MRCAL_AMD_TM_CCORR_NORMED  3
#define MRCAL_AMD_TM_CCOEFF        4
#define MRCAL_AMD_TM_CCOEFF_NORMED 5
typedef struct mrcal_amd_feature_matcher mrcal_amd_feature_matcher_t;
mrcal_amd_feature_matcher_t*
mrcal_amd_feature_matcher_create(const void* image0, int width0, int height0,
                                 const void* image1, int width1, int height1, int dtype);
bool mrcal_amd_feature_matcher_match(mrcal_amd_feature_matcher_t* m, int N,
                                     const double* q1_estimate /*N,2*/, const double* H01 /*N,3,3*/,
                                     int template_width, int template_height, int search_radius, int method,
                                     double* q1 /*N,2*/, int* status /*N*/,
                                     double* optimum_subpixel_at /*N,2*/, double* optimum_subpixel /*N*/,
                                     int* qmin /*N,2*/, int* output_size /*N,2*/);
bool mrcal_amd_feature_matcher_matchoutput(mrcal_amd_feature_matcher_t* m, int i, float* matchoutput);
bool mrcal_amd_feature_matcher_template(mrcal_amd_feature_matcher_t* m, int i, void* template_image);
void mrcal_amd_feature_matcher_destroy(mrcal_amd_feature_matcher_t* m);

/* ---- stereo_matching_sgm: dense disparities of a rectified pair -------------
   The step between mrcal_amd_rectification_rectify() and mrcal_amd_rectification_range(), for which the reference's
   tool leaves the library (cv2.StereoSGBM, mrcal.stereo_matching_libelas()): a semi-global matcher on a census cost,
   csrc/stereo_sgm.hip, planned on the host by csrc/sgm_plan.hpp. Integer arithmetic throughout and no atomics: the
   result is defined to the bit, and is the same bits on every call.

   image0 (left) and image1 (right): rectified, one channel, dense, the same (H,W) and dtype, MRCAL_AMD_IMAGE_UINT8 or
   _UINT16. D = disparity_max - disparity_min is a positive multiple of 16, at most 256; disparity_min may be
   negative. The index i in [0,D) means the disparity d = disparity_min + i.
     1. Census. Per image and pixel a 62-bit descriptor over the window 9 wide x 7 tall around the pixel, the centre
        left out: a bit is (neighbour < centre). A neighbour outside the image is the nearest pixel inside (clamped
        coordinates). Only Hamming distances are used: the order of the bits is free
     2. Cost. C(y,x,i) = popcount(census0(y,x) XOR census1(y,x-d)); 62 where x-d is outside [0,W)
     3. Aggregation. For each path direction r, with m = min_k L_r(p-r,k):
          L_r(p,i) = C(p,i) + min(L_r(p-r,i), L_r(p-r,i-1) + P1, L_r(p-r,i+1) + P1, m + P2) - m
        An i-1 or i+1 outside [0,D) takes no part. Where p-r is outside the image, L_r(p,.) = C(p,.). paths = 4:
        (0,+-1), (+-1,0); paths = 8: the four diagonals too. S = sum_r L_r. 0 <= P1 <= P2 <= 193, so that
        L_r <= 62 + P2 <= 255 and S <= 2040
     4. Selection. i* = the FIRST index of the minimum of S(p,.). The pixel is invalid if some i with |i - i*| > 1 has
        S(p,i) (100 - uniqueness_ratio) < S(p,i*) 100 (uniqueness_ratio in 0..99; 0: no test). The scaled index is
        16 i*, and where 0 < i* < D-1, with a = S(i*-1), c = S(i*+1), den = max(a + c - 2 S(i*), 1):
        16 i* + floor(((a - c) 16 + den)/(2 den)), a FLOOR of a numerator that may be negative
     5. Left-right check; disp12_max_diff < 0: none. The right image's index i1(y,x1) = the smallest i that minimises
        S(y, x1 + d, i) over the i whose x1 + d is inside the image. A left pixel is invalid if x - d* is outside the
        image, or if |i1(y, x - d*) - i*| > disp12_max_diff
     6. disparity: int16 (H,W): 16 disparity_min + the scaled index; an invalid pixel holds 16 (disparity_min - 1).
        A range whose scaled values leave int16 is refused. The scale is cv2's: MRCAL_AMD_STEREO_SGM_DISPARITY_SCALE
   Not here: cv2's Birchfield-Tomasi cost on Sobel-filtered images, its adaptive P2, colour input, ELAS.
   _create(): the handle owns every device buffer a match of that size needs (a problem that does not fit the free
   device memory is refused with its size); _match(): host arrays in and out; _stage_milliseconds(): how long the
   census, the paths, the selection and the left-right check of the last _match() took on the device (4 values).
   mrcal_amd_rectification_disparity(): the two images are rectified (linear interpolation, 0 outside) into device
   buffers and matched there: the rectified images do not cross to the host and back.
   The speckle filter ("filter_speckles", below) is a stage of its own after step 6, on request only:
   _set_speckle_filter(m, window_size, range), cv2.StereoSGBM's speckleWindowSize and speckleRange. window_size = 0
   (what a new matcher has): no filter, nothing of it runs and the result is that of steps 1-6. window_size > 0: every
   later _match() filters the disparity image on the device before it is copied out, with new_value =
   16 (disparity_min - 1), max_speckle_size = window_size, max_diff = 16 range. The labels and counts lie in S, which is
   dead by then: the matcher allocates nothing more. _speckle_milliseconds(): how long that stage of the last _match()
   took (0 without the filter); _stage_milliseconds() keeps its 4 values.
   mrcal_amd_rectification_disparity_filtered() is mrcal_amd_rectification_disparity() with the two integers */
#define MRCAL_AMD_STEREO_SGM_DISPARITY_SCALE 16
typedef struct
{
    int disparity_min, disparity_max;   /* 0, required */
    int P1, P2;                         /* 10, 120 */
    int paths;                          /* 8 */
    int uniqueness_ratio;               /* 10 */
    int disp12_max_diff;                /* 1 */
} mrcal_amd_stereo_sgm_params_t;
typedef struct mrcal_amd_stereo_sgm mrcal_amd_stereo_sgm_t;
mrcal_amd_stereo_sgm_t*
mrcal_amd_stereo_sgm_create(int width, int height, int dtype, const mrcal_amd_stereo_sgm_params_t* params);
bool mrcal_amd_stereo_sgm_match(mrcal_amd_stereo_sgm_t* m, const void* image0, const void* image1, int16_t* disparity);
bool mrcal_amd_stereo_sgm_stage_milliseconds(mrcal_amd_stereo_sgm_t* m, float* milliseconds /*4*/);
void mrcal_amd_stereo_sgm_destroy(mrcal_amd_stereo_sgm_t* m);
bool mrcal_amd_rectification_disparity(mrcal_amd_rectification_t* r,
                                       const void* image0, int width0, int height0,
                                       const void* image1, int width1, int height1, int dtype,
                                       const mrcal_amd_stereo_sgm_params_t* params, int16_t* disparity);
bool mrcal_amd_stereo_sgm_set_speckle_filter(mrcal_amd_stereo_sgm_t* m, int window_size, int range);
bool mrcal_amd_stereo_sgm_speckle_milliseconds(mrcal_amd_stereo_sgm_t* m, float* milliseconds /*1*/);
bool mrcal_amd_rectification_disparity_filtered(mrcal_amd_rectification_t* r,
                                                const void* image0, int width0, int height0,
                                                const void* image1, int width1, int height1, int dtype,
                                                const mrcal_amd_stereo_sgm_params_t* params,
                                                int speckle_window_size, int speckle_range, int16_t* disparity);

/* ---- filter_speckles: small regions of a disparity image become invalid ------
   cv2.filterSpeckles(img, newVal, maxSpeckleSize, maxDiff) for CV_16S, which cv2.StereoSGBM applies to its result and
   the reference's mrcal-stereo tool recommends (--sgbm-speckle-window-size 200 --sgbm-speckle-range 2); here it is
   csrc/speckle_filter.hip, planned on the host by csrc/speckle_plan.hpp. On an int16 image (H,W), dense:
     1. A pixel equal to new_value takes no part and is never changed
     2. Two 4-neighbours (left/right, up/down) that both take part are joined if |a - b| <= max_diff. The difference is
        taken in 32 bits: -32768 beside 32767 differs by 65535. A max_diff above 65535 means 65535
     3. The regions are the connected components of that graph
     4. Every pixel of a region of size <= max_speckle_size becomes new_value; everything else is unchanged.
        max_speckle_size = 0 changes nothing
   Only original values are compared and the relation is symmetric, so the result does not depend on the order in
   which cv2's flood fill, or anything else, visits the pixels. "Equal to cv2" rests on a transcription of cv2's loop
   (tests/speckle_checker.py: filter_speckles_loops()) that a graph formulation is held to, not on cv2 itself.
   Connected-component labelling by union-find: a label is an int32 pixel index, two roots are joined by pointing the
   larger at the smaller, so a region's root is its smallest index and a region's size an integer sum: integer atomics
   whose result does not depend on the order, no floating point, the same bits on every call.
   Refused: an image that is empty or has more than 2^28 pixels, a new_value outside int16, a negative
   max_speckle_size or max_diff, an image that does not fit the free device memory (10 bytes a pixel).
   _create(): the handle owns ONE device allocation for images of that size; _apply(): host arrays, in == out is
   allowed; _milliseconds(): how long the last _apply() took on the device, without the copies;
   _pass_milliseconds(): the same pass by pass (4 values: the tiles' labels, the joins across the tiles' borders, the
   roots and sizes, the result) */
typedef struct mrcal_amd_speckle_filter mrcal_amd_speckle_filter_t;
mrcal_amd_speckle_filter_t* mrcal_amd_speckle_filter_create(int width, int height);
bool mrcal_amd_speckle_filter_apply(mrcal_amd_speckle_filter_t* f, const int16_t* in, int16_t* out,
                                    int new_value, int max_speckle_size, int max_diff);
bool mrcal_amd_speckle_filter_milliseconds(mrcal_amd_speckle_filter_t* f, float* milliseconds /*1*/);
bool mrcal_amd_speckle_filter_pass_milliseconds(mrcal_amd_speckle_filter_t* f, float* milliseconds /*4*/);
void mrcal_amd_speckle_filter_destroy(mrcal_amd_speckle_filter_t* f);

/* ---- stereo_point_cloud: disparities to a compacted, coloured cloud of points ----
   What the reference's mrcal-stereo --write-point-cloud delivers, from the disparities a matcher left on the device:
   csrc/point_cloud.hip, planned on the host by csrc/point_cloud_plan.hpp. Only the kept points cross to the host.
   A pixel (x,y) of the dense (Nel,Naz) disparity image is KEPT when all of these hold:
     1. Disparity. With d the disparity cast to uint16, as mrcal_stereo_range_dense() takes it: d > 0,
        d >= disparity_scaled_min, d <= disparity_scaled_max (for an int16 image the maximum defaults to 0x7FFF, so that
        its negative "invalid" marks stay invalid)
     2. Range. range = the range mrcal_stereo_range_dense() gives for d/disparity_scale at (x,y), from the same device
        function, is finite and > 0. A negative LATLON range, which mrcal_stereo_range_dense() returns, is dropped here
     3. Range limits. range_min <= range <= range_max (0 and infinity: no limits)
     4. Colour pixel, if a colour image of camera 0 is given. With (mx,my) the float32 rectification map of camera 0 at
        (x,y): ix = floorf(mx + 0.5f), iy = floorf(my + 0.5f), the additions in float32, are finite and inside the
        image. The colour is image[iy, ix]: the reference's "nearest pixel of the original image", from the map the
        rectification holds instead of a projection of every point. Departure: a map entry of -0.5 exactly is inside
        here (pixel 0) and outside in the reference
   The point is p_rect0 = range v, v the unit observation vector of the rectified pixel (LATLON: (sin az, cos az sin el,
   cos az cos el); PINHOLE: (ux, uy, 1)/|.|), and p = R p_rect0 + t with Rt_out_rect0 (4,3) = R, then t, made on the host.
   Rt_out_rect0 = NULL: p = p_rect0 and no product is made, so that the points carry the bits of
   mrcal_amd_stereo_range_sparse()'s p. The arithmetic is in double; a point is stored as float64 or, rounded once at
   the store, as float32 (what a .ply holds).
   Order: the kept pixels appear in ascending linear index y Naz + x. The outputs: points (N,3); color (N,) or (N,3) of
   the image's type (uint8 or uint16; 1 or 3 interleaved channels); index (N,) int32, the linear index of each point.
   Deterministic: validity is decided ONCE, by cloud_mask_kernel, and stored a bit a pixel; an integer scan of the
   per-workgroup counts gives every workgroup its place; cloud_scatter_kernel reads the bits. No atomics, no workgroup
   waits for another, the same bits on every call.
   Refused: an image that is empty or has more than 2^28 pixels or does not fit the free device memory,
   disparity_scaled_min >= disparity_scaled_max, range_min > range_max or not a number, a colour image that is not
   uint8 or uint16 with 1 or 3 channels, a colour image without a map.
   Two calls: _compute() uploads the disparities (host, dense) and the colour image, runs the kernels and returns N;
   _read() copies the N records into the caller's arrays, any of which may be NULL. The output buffers on the device
   are kept from call to call and grow when N outgrows them (csrc/point_cloud_plan.hpp: cloud_capacity()).
   _create(): device_map0: the rectification map of camera 0 ON THE DEVICE, (Nel,Naz,2) float32, aligned to 16 bytes,
   which must outlive the object; NULL: none (no colours then). _set_map(): a map of the HOST's instead, copied.
   _stage_milliseconds(): how long the mask, the scan and the scatter of the last _compute() took on the device.
   mrcal_amd_rectification_point_cloud*(): the same through the object a rectification owns, with its map of camera 0;
   _of_images() rectifies the pair, matches it (and filters the speckles: "stereo_matching_sgm") and makes the cloud
   without the rectified images or the disparities leaving the device. There the disparity fields of the parameters
   are the matcher's and are not read: scale 16, minimum 16 disparity_min, maximum 0x7FFF; a negative disparity_min is
   refused, as the cast to uint16 has no meaning for negative disparities */
typedef struct mrcal_amd_point_cloud mrcal_amd_point_cloud_t;
typedef struct
{
    uint16_t      disparity_scale, disparity_scaled_min, disparity_scaled_max;
    double        range_min, range_max;         /* 0 and INFINITY: no limits */
    const double* Rt_out_rect0;                 /* (4,3) or NULL */
    int           points_float32;               /* the points are stored as float32, not float64 */
    const void*   image;                        /* the colour image of camera 0, dense, on the host; NULL: no colours */
    int           image_width, image_height, image_channels, image_dtype;      /* MRCAL_AMD_IMAGE_UINT8 or _UINT16 */
} mrcal_amd_point_cloud_params_t;
mrcal_amd_point_cloud_t*
mrcal_amd_point_cloud_create(const mrcal_lensmodel_type_t rectification_model_type, const double* fxycxy_rectified,
                             double baseline, int width, int height, const float* device_map0);
bool mrcal_amd_point_cloud_set_map(mrcal_amd_point_cloud_t* c, const float* map0);
bool mrcal_amd_point_cloud_compute(mrcal_amd_point_cloud_t* c, const uint16_t* disparity_scaled,
                                   const mrcal_amd_point_cloud_params_t* params, int* N);
bool mrcal_amd_point_cloud_read(mrcal_amd_point_cloud_t* c, void* points, void* color, int32_t* index);
bool mrcal_amd_point_cloud_stage_milliseconds(mrcal_amd_point_cloud_t* c, float* milliseconds /*3*/);
void mrcal_amd_point_cloud_destroy(mrcal_amd_point_cloud_t* c);
bool mrcal_amd_rectification_point_cloud(mrcal_amd_rectification_t* r, const uint16_t* disparity_scaled,
                                         const mrcal_amd_point_cloud_params_t* params, int* N);
bool mrcal_amd_rectification_point_cloud_of_images(mrcal_amd_rectification_t* r,
                                                   const void* image0, int width0, int height0,
                                                   const void* image1, int width1, int height1, int dtype,
                                                   const mrcal_amd_stereo_sgm_params_t* sgm_params,
                                                   int speckle_window_size, int speckle_range,
                                                   const mrcal_amd_point_cloud_params_t* params, int* N);
bool mrcal_amd_rectification_point_cloud_read(mrcal_amd_rectification_t* r, void* points, void* color, int32_t* index);
bool mrcal_amd_rectification_point_cloud_stage_milliseconds(mrcal_amd_rectification_t* r, float* milliseconds /*3*/);

/* ---- chessboard corners: the calibration board detected in one grey image ----
   What the reference gets from an external detector (mrgingham) through mrcal.compute_chessboard_corners():
   csrc/chessboard.hip, planned on the host by csrc/chessboard_plan.hpp; the lattice is found on the host by
   csrc/chessboard_grid.cpp. It imitates no other detector pixel for pixel; it finds the same physical corners.
   The image I: grey, uint8 or uint16, (H,W), dense rows. All of a..c is integer arithmetic.
     a. Blur. B = I (*) [1 2 1]^T [1 2 1], the plain integer sum: B <= 16 max(I). Nothing is divided
     b. Response: the ChESS detector of Bennett & Lasenby. The ring s[0..15] is B at the offsets (dx,dy)
          (5,0) (5,2) (3,3) (2,5) (0,5) (-2,5) (-3,3) (-5,2) (-5,0) (-5,-2) (-3,-3) (-2,-5) (0,-5) (2,-5) (3,-3) (5,-2)
          SR  = sum_{n<4} |(s[n] + s[n+8]) - (s[n+4] + s[n+12])|
          DR  = sum_{n<8} |s[n] - s[n+8]|
          S16 = sum s          S5 = B(p) + B at its four 4-neighbours
          R   = 5 SR - 5 DR - |5 S16 - 16 S5|          as an int32: the paper's sum - diff - 16 mean response, times 5
        For uint16 input every intermediate stays below 2^27. R is this for 6 <= x < W-6 and 6 <= y < H-6 and 0
        elsewhere: no coordinate is ever clamped
     c. Candidates. Rmax = max R over the image (>= 0: the border). A pixel p is a candidate when R(p) > 0, and
        256 R(p) > threshold_256 Rmax (a 64-bit product), and for every other p' of the (2 nms_radius + 1)^2 window
        inside the image R(p') < R(p), or R(p') == R(p) and p' comes after p in row-major order. The candidates are
        listed in row-major order; the first max_candidates of them are kept and the rest counted: overflow
     d. Refinement, on I in double: the fixed point of cv2.cornerSubPix. q = (x,y) of the candidate; the window offsets
        i,j in [-5,5] with weights exp(-(i/5)^2) exp(-(j/5)^2); I sampled bilinearly at coordinates clamped to the image
        (x to [0,W-1]: x0 = floor(x), x1 = min(x0 + 1, W-1)); gx = (I(q+(i+1,j)) - I(q+(i-1,j)))/2, gy likewise;
        G = sum w g g^T; singular when !(det G > 1e-10 (trace G)^2): status 1; d = G^-1 sum w g g^T (i,j)^T; q += d;
        |q - start| > 3.5 px along x or y: status 2; stop when |d| < 1e-5 px or after 20 iterations: status 0. A
        candidate that fails has NaN coordinates
     e. The board: the complete width x height lattice (3..256 corners a side) among the refined candidates of status
        0, or none (whole boards only, like mrgingham). Row-major, (height,width,2). The labelling is proper: with the image's y pointing down,
        (mean +i edge) x (mean +j edge) > 0, +i along a row and +j along a column of the board. Of the 2 proper
        labellings (4 when width == height) the one whose mean +i edge, made a unit vector, has the largest x
   Deterministic: the maximum is an INTEGER atomicMax; the compaction is point_cloud.hip's (a mask bit a pixel, one
   integer scan, a scatter from the bits); the sums of d are reduced in a fixed order. The same bits on every call.
   Refused: bytes_per_pixel other than 1 or 2, an image smaller than 32 x 32 or of more than 2^28 pixels or that does
   not fit free_device_bytes, threshold_256 outside 0..255, nms_radius outside 1..16, max_candidates outside 1..65536.
   _create(): free_device_bytes: what the device has free; 0: ask it. _candidates(): uploads the image (host, dense),
   runs a..d, returns how many candidates are kept (*N) and whether more were found (*overflow); the caller's arrays
   q (N,2) double, response (N,) int32, status (N,) int32 hold max_candidates entries and may be NULL. _find_board():
   _candidates() and e; *found = 0: no board, which is no error. _stage_milliseconds(): upload, response, candidates,
   refine (the device's events), grid (the host's clock; 0 after _candidates()) of the last call.
   mrcal_amd_chessboard_grid(): e alone, on the host, for N points that are given: it needs no device. response
   orders the seeds (NULL: the order given), status NULL: all 0

   The image pyramid (opt-in: pyramid_levels = n > 0; with n = 0 everything above is all there is, to the bit). For
   corners that are blurred over several pixels, or boards whose squares cover hundreds of pixels: a..e at one scale
   see them badly or not at all. What mrgingham's decimation level is in the reference.
     p1. Decimation. Level 0 is I. Level l+1 has floor(W_l/2) x floor(H_l/2) pixels,
           I_{l+1}(x,y) = (I_l(2x,2y) + I_l(2x+1,2y) + I_l(2x,2y+1) + I_l(2x+1,2y+1) + 2) >> 2
         in integers, the same for uint8 and uint16; an odd last row or column is dropped. A point q of level l+1 lies
         at up(q) = 2 q + 0.5 of level l. pyramid_levels = n asks for the levels 0..n, n in 0..8; every level has at
         least 32 pixels a side, so n <= the largest n with min(W >> n, H >> n) >= 32, and a larger one is refused
         with that number in the message
     p2. Where the board is looked for: coarsest first. For L = n, n-1, .., 0: a..e on I_L, with the same
         threshold_256, nms_radius and max_candidates, in pixels of level L. The first L at which e yields a complete
         board is the detection level; no such L: no board
     p3. Descent, each corner on its own. A corner starts with level L and its position q_L there. For l = L-1 .. 0 a
         corner whose level is l+1 is refined on I_l by d, started from the FLOAT up(q_{l+1}): the window, the
         weights, the 20 iterations and the stop rule are d's, and "left" is +-3.5 px around that start. The corner
         moves to level l (position: the refined point) when the status is 0 and max(|dx|,|dy|) <= tau between the
         refined point and its start, in pixels of level l; otherwise it stays where it is for good. Reported: the
         last accepted position carried to level 0 by repeated up(), and the level it was accepted at
     tau = 0.3 px (CB_DESCENT_AGREEMENT in csrc/chessboard_plan.hpp). Measured with the numpy checker
     (tests/chessboard_pyramid_checker.py) on rendered 7 x 5 boards of 30, 60 and 110 px squares turned by 17 degrees,
     noise of 1 grey level, then a Gaussian blur of sigma px: with sigma <= 3 every step of every corner disagrees by
     at most 0.200 px (reached at sigma = 0) and every corner reaches level 0; at sigma = 4 the steps to level 0 disagree
     by 0.003 .. 0.66 px with nothing between that separates good from bad, and tau = 0.3 brings 17 or 18 of 35 corners
     to level 0; at sigma = 6 every refinement on level 0 leaves its box (status 2) and every corner stays at level 1.
     So tau stays at the 0.3 px it was proposed with (the table).
     The level is what mrcal.compute_chessboard_corners() reads as the weight 2^-level.
   _create_pyramid(): _create() and pyramid_levels; the pool grows by the level images (1/3 of the image) and the
   board's corner records. _find_board_pyramid(): uploads the image, makes the levels, p2 and p3; corners
   (board_height, board_width, 2) in level-0 pixels, levels (board_height, board_width) int32, *detection_level (-1:
   not found). On a detector with pyramid_levels = 0: _find_board()'s corners to the bit, levels 0. _candidates() and
   _find_board() of a detector with levels look at level 0 alone. _read_response() and _stage_milliseconds() speak
   of the level that was looked at last: the detection level, or 0 when no board was found (the upload is the one of
   the image). _read_level(): the image of a level as the last call left it, dense, of the image's type (levels above
   0 exist after _find_board_pyramid()). _pyramid_milliseconds(): the decimation and the descent by the device's
   events; per_level [pyramid_levels + 1]: the host's clock around each level tried (a..e and the read-back of its
   candidates), 0 for a level that was not tried */
typedef struct mrcal_amd_chessboard_detector mrcal_amd_chessboard_detector_t;
typedef struct
{
    int threshold_256;          /* 51 */
    int nms_radius;             /* 7 */
    int max_candidates;         /* 4096 */
} mrcal_amd_chessboard_params_t;
#define MRCAL_AMD_CHESSBOARD_STAGES 5
mrcal_amd_chessboard_detector_t*
mrcal_amd_chessboard_detector_create(int width, int height, int bytes_per_pixel,
                                     const mrcal_amd_chessboard_params_t* params, size_t free_device_bytes);
bool mrcal_amd_chessboard_detector_candidates(mrcal_amd_chessboard_detector_t* d, const void* image,
                                              int* N, int* overflow, double* q, int32_t* response, int32_t* status);
bool mrcal_amd_chessboard_detector_find_board(mrcal_amd_chessboard_detector_t* d, const void* image,
                                              int board_width, int board_height, int* found, double* corners);
/* for the tests: the response image (height,width) int32, Rmax and the pixels (N,2) of the candidates of the last call;
   any of them may be NULL */
bool mrcal_amd_chessboard_detector_read_response(mrcal_amd_chessboard_detector_t* d, int32_t* response, int32_t* response_max,
                                                 int32_t* candidate_xy);
bool mrcal_amd_chessboard_detector_stage_milliseconds(mrcal_amd_chessboard_detector_t* d, float* milliseconds /*5*/);
void mrcal_amd_chessboard_detector_destroy(mrcal_amd_chessboard_detector_t* d);
#define MRCAL_AMD_CHESSBOARD_MAX_PYRAMID_LEVELS 8
mrcal_amd_chessboard_detector_t*
mrcal_amd_chessboard_detector_create_pyramid(int width, int height, int bytes_per_pixel,
                                             const mrcal_amd_chessboard_params_t* params, int pyramid_levels,
                                             size_t free_device_bytes);
bool mrcal_amd_chessboard_detector_find_board_pyramid(mrcal_amd_chessboard_detector_t* d, const void* image,
                                                      int board_width, int board_height, double* corners,
                                                      int32_t* levels /* [board_height*board_width] */,
                                                      int* detection_level, int* found);
bool mrcal_amd_chessboard_detector_read_level(mrcal_amd_chessboard_detector_t* d, int level, void* image_out);
bool mrcal_amd_chessboard_detector_pyramid_milliseconds(mrcal_amd_chessboard_detector_t* d, float* decimate, float* descent,
                                                        float* per_level /* [pyramid_levels + 1] */);
bool mrcal_amd_chessboard_grid(int N, const double* q, const int32_t* response, const int32_t* status,
                               int board_width, int board_height, int* found, double* corners);

/* ---- equalization: CLAHE and stretch of a grey image, before it is rectified and matched ----
   What the reference's tools do to every raw image first: mrcal-stereo --equalization {clahe,stretch} and
   mrcal-triangulate --clahe through cv2.createCLAHE(), setClipLimit(8), apply(); mrcal_image_uint8_load() stretches a
   16-bit image to 8 bits. Here it is csrc/equalize.hip, planned on the host by csrc/equalize_plan.hpp.
   cv2 is no part of this project: what follows is the published algorithm of OpenCV's clahe.cpp, quirks included, and
   this text is the authority. Equality with cv2 itself is NOT tested. tests/equalize_checker.py restates it twice.

   CLAHE. The image: grey, dense (H,W), uint8 (histSize = 256) or uint16 (histSize = 65536); the result has its shape
   and type. clip_limit (8.0 is mrcal's value; <= 0: nothing is clipped); tiles_x, tiles_y (8, 8).
     1. Padding. None if W % tiles_x == 0 and H % tiles_y == 0. Otherwise the image is padded on the right by
        tiles_x - W % tiles_x and at the bottom by tiles_y - H % tiles_y, BOTH, even where one side is divisible: that
        side gets a whole tiles_x (tiles_y) more. The padding is BORDER_REFLECT_101 (numpy.pad(mode='reflect')): the
        pixel at index W-1+k is the one at W-1-k. The padded image is never made on the device: a padded pixel is
        read at its reflected index
     2. tw = Wpad/tiles_x, th = Hpad/tiles_y, total = tw th; lutScale = float32(histSize - 1) / float32(total);
        clip = max(int(clip_limit total / histSize), 1), the product and the quotient in double, truncated
     3. Per tile of the padded image: h = its histogram; clipped = sum_i max(h[i] - clip, 0); h[i] = min(h[i], clip);
        batch = clipped / histSize, residual = clipped - batch histSize (integers); every h[i] += batch; if
        residual > 0: step = max(histSize / residual, 1), and h[i] += 1 for i = 0, step, 2 step, ... while
        i < histSize and fewer than residual bins have been incremented (bin i: i % step == 0 and i/step < residual);
        lut[i] = saturate(rint(float32(sum_{k<=i} h[k]) lutScale)), the sum an integer, rint halves to even
     4. Per pixel (x,y) of the image (not of the padding), with value v, in float32, EVERY operation rounded on its
        own (nothing is fused): txf = float32(x) (1.f/float32(tw)) - 0.5f; tx1 = floor(txf); xa = txf - tx1;
        xa1 = 1.f - xa; then tx1 and tx2 = tx1 + 1 are clamped to [0, tiles_x - 1]. The same in y.
          res = (lut[ty1][tx1][v] xa1 + lut[ty1][tx2][v] xa) ya1 + (lut[ty2][tx1][v] xa1 + lut[ty2][tx2][v] xa) ya
        The result is saturate(rint(res)), halves to even
   Stretch. uint8 or uint16 in, uint8 out: out = uint8(0.5f + float32(v - min) 255.f / float32(max - min)), the
   product before the quotient, in float32, truncated; min and max over the whole image, as integers. Departures from
   image.c: its loop misses a maximum that comes before the first smaller pixel (the true extremes are used here), and
   it divides by zero for a constant image (here: all zeros).
   Histograms are integer sums and the extremes integer minima and maxima: integer atomics whose result does not depend
   on the order, no floating-point atomic anywhere, the same bits on every call.
   Refused: a method or type that is none of the above, an image that is empty or has more than 2^28 pixels, tiles
   below 1 or more than 4096 in all, a clip_limit that is not a number, an image so small that the padding exceeds
   W-1 or H-1 (a reflection reaches no further), an image that does not fit the free device memory.
   _create(): the handle owns ONE device allocation: the image, the result, the histograms, the LUTs. _apply(): host
   arrays, dense. _stage_milliseconds(): how long the histograms, the LUTs and the interpolation of the last _apply()
   took on the device (stretch: the extremes, 0, the map).
   mrcal_amd_rectification_set_equalization(): MRCAL_AMD_EQUALIZE_NONE (what a new handle has): nothing of this runs
   and every result is what it was. Otherwise every later _rectify(), _disparity(), _disparity_filtered() and
   _point_cloud_of_images() equalizes each raw image on the device between its upload and the remap; the images are
   then grey. With stretch the rectified images, and the matcher, are uint8 whatever the input. In
   _point_cloud_of_images() a colour image that IS image0 (the same pointer and size, one channel) is taken equalized,
   from where it lies on the device; any other is used as it is.
   mrcal_amd_feature_matcher_create_equalized(): _create(), both images equalized on the device after the upload
   (uint8 or uint16 then; with stretch the templates are uint8) */
#define MRCAL_AMD_EQUALIZE_NONE    0
#define MRCAL_AMD_EQUALIZE_CLAHE   1
#define MRCAL_AMD_EQUALIZE_STRETCH 2
typedef struct
{
    int    method;              /* MRCAL_AMD_EQUALIZE_* */
    double clip_limit;          /* 8.0 */
    int    tiles_x, tiles_y;    /* 8, 8 */
} mrcal_amd_equalize_params_t;
typedef struct mrcal_amd_equalizer mrcal_amd_equalizer_t;
mrcal_amd_equalizer_t* mrcal_amd_equalizer_create(int width, int height, int dtype, const mrcal_amd_equalize_params_t* params);
bool mrcal_amd_equalizer_apply(mrcal_amd_equalizer_t* e, const void* in, void* out);
bool mrcal_amd_equalizer_stage_milliseconds(mrcal_amd_equalizer_t* e, float* milliseconds /*3: histogram, lut, apply*/);
void mrcal_amd_equalizer_destroy(mrcal_amd_equalizer_t* e);
bool mrcal_amd_rectification_set_equalization(mrcal_amd_rectification_t* r, const mrcal_amd_equalize_params_t* params);
mrcal_amd_feature_matcher_t*
mrcal_amd_feature_matcher_create_equalized(const void* image0, int width0, int height0,
                                           const void* image1, int width1, int height1, int dtype,
                                           const mrcal_amd_equalize_params_t* params);

/* ---- smoothing: a separable Gaussian of a grey image, before it is remapped to fewer pixels ----
   A remap reads 4 pixels of its source for a pixel of its result, whatever the scale: one that makes the image 3-8 x
   smaller, as the rectification of a large pair to the matcher's disparity range does, drops most of the image and
   aliases the rest. The reference's to-do list has the entry (doc/news-3.0.org: "mrcal-stereo should have an
   anti-aliasing filter ... when I downsample, just before mrcal.transform_image()", with cv2.GaussianBlur(sigmaX = 2)),
   which it never built. Here it is csrc/smooth.hip, planned on the host by csrc/smooth_plan.hpp. cv2 is no part of
   this project and no equality with cv2.GaussianBlur() is claimed: this text is the authority, and
   tests/smooth_checker.py restates it twice.

   The image: grey, dense (H,W), uint8 or uint16; the result has its shape and type. sigma_x, sigma_y: each is 0 (that
   axis is not filtered) or lies in [0.5, 8].
   Taps, per axis, from its sigma:
     1. R = ceil(3 sigma), so R <= 24; g_k = exp(-k^2 / (2 sigma^2)) for k = 0..R, in double
     2. S = g_0 + 2 sum_{k>=1} g_k; a_k = 256 g_k / S
     3. integer weights by error diffusion from the outside in: e = 0; for k = R, R-1, ..., 1:
        w_k = floor(a_k + e + 0.5), then e += a_k - w_k. Last w_0 = 256 - 2 sum_{k>=1} w_k, and w_-k = w_k
     4. sigma = 0: the single tap w_0 = 256
   They sum to 256, 0 <= w_k <= 255 for every sigma in [0.5, 8], and |w_k - a_k| <= 1; above sigma ~ 3.3 they are not
   monotone in k: eight bits are too coarse for that.
   Arithmetic: integers only; a coordinate outside the image is clamped to it (the border is replicated).
     horizontal   T[y][x] = sum_k wx_k I[y][clamp(x + k)]                         no rounding, no shift
     vertical     O[y][x] = (sum_k wy_k T[clamp(y + k)][x] + 32768) >> 16
   The largest value, of a uint16 image, is 65535 256 256 + 32768 = 2^32 - 32768: an unsigned 32-bit accumulator holds
   it. A constant image comes back unchanged. No floating point on the device and no atomics: the same bits on every
   call.
   Refused: a sigma that is neither 0 nor in [0.5, 8] (a NaN is neither), both sigmas 0 (there is nothing to run), a type
   that is neither uint8 nor uint16, an image that is empty or has more than 2^28 pixels, an image that does not fit
   the free device memory.
   _create(): the handle owns ONE device allocation: the image and the result. _apply(): host arrays, dense.
   _milliseconds(): how long the one launch of the last _apply() took on the device, without the copies.
   mrcal_amd_smooth_weights(): R and w_0..w_R of one sigma (0, or > 0 with R <= 24), on the host: no device is needed.
   mrcal_amd_rectification_set_antialias(): NULL or both sigmas 0 (what a new handle has): nothing of this runs and
   every result is what it was. Otherwise every later _rectify(), _disparity(), _disparity_filtered() and
   _point_cloud_of_images() filters each raw image on the device, after its upload and after its equalization if one is
   set, before the remap; the images are then grey, uint8 or uint16. The colours of _point_cloud_of_images() are NOT
   filtered: they come from the image as it was before the filter.
   mrcal_amd_transform_image_smoothed(): mrcal_amd_transform_image() of the image filtered so, on the device between the
   upload and the remap; params NULL or both sigmas 0: mrcal_amd_transform_image() */
typedef struct
{
    double sigma_x, sigma_y;    /* each 0, or in [0.5, 8] */
} mrcal_amd_smooth_params_t;
typedef struct mrcal_amd_smoother mrcal_amd_smoother_t;
mrcal_amd_smoother_t* mrcal_amd_smoother_create(int width, int height, int dtype, const mrcal_amd_smooth_params_t* params);
bool mrcal_amd_smoother_apply(mrcal_amd_smoother_t* s, const void* in, void* out);
bool mrcal_amd_smoother_milliseconds(mrcal_amd_smoother_t* s, float* milliseconds);
void mrcal_amd_smoother_destroy(mrcal_amd_smoother_t* s);
bool mrcal_amd_smooth_weights(double sigma, int* R, int* w /* up to 25: w_0..w_R */);
bool mrcal_amd_rectification_set_antialias(mrcal_amd_rectification_t* r, const mrcal_amd_smooth_params_t* params);
bool mrcal_amd_transform_image_smoothed(void* out, const void* image, int width, int height, int channels, int dtype,
                                        const float* mapxy, int width_out, int height_out,
                                        int interpolation, int border_mode, const double* border_value,
                                        const mrcal_amd_smooth_params_t* params);

/* ---- regional statistics: the residuals of a solve, binned over a grid of each imager ----
   What mrcal-calibrate-cameras looks at between the solve and the .cameramodel file (mrcal/calibration.py:1720-1866,
   _report_regional_statistics()). Here it is csrc/regional_stats.hip, planned on the host by
   csrc/regional_stats_plan.hpp, all the cameras of a problem in one pass. This text is the authority;
   tests/valid_region_checker.py restates it in plain loops.

   The inputs are the problem's: x at its current state (the board measurements, weighted as they are in x), the
   board observations (qx, qy, weight) and the camera of each. Camera c has an imager of W x H pixels and a grid of
   gridn_width x gridn_height cells; gridn_height <= 0: int(round(H/W*gridn_width)), the product (H/W)*gridn_width in
   double, halves to even, for each camera by its own imager. Both must be >= 2.
     - the centres: cx[i] = i*((W-1)/(gridn_width-1)) for i < gridn_width-1, one division and one multiplication in
       double, and cx[gridn_width-1] = W-1; cy[j] likewise from H and gridn_height: np.linspace(), and
       sample_imager(). wcell = (W-1)/(gridn_width-1), hcell = (H-1)/(gridn_height-1)
     - a corner takes part if its weight is > 0. It is in cell (i,j) of its camera iff |qx - cx[i]| < wcell/2 and
       |qy - cy[j]| < hcell/2, each a subtraction, an absolute value and a comparison in double, both strict: a corner
       on a border between cells is in neither, a corner beyond the outermost half cells in none. Every cell is
       asked on its own, as the reference asks: with the centres rounded, a corner within an ulp of a border can meet
       the inequalities of both cells beside it, and then it is in both
     - per cell, over the x and y residuals of its corners pooled, n values (even): count = n; n <= 5: mean = stdev =
       0; else mean = sum/n and stdev = sqrt(sum((v - mean)^2)/n), the population deviation in two passes
     - the order of the sums: the cell's corners in ascending measurement index, value v = 2k the x and v = 2k+1 the
       y residual of its k-th corner; lane l of 64 adds the values l, l+64, l+128, ... in that order, the 64 lanes are
       added by the butterfly s += s[lane ^ 32], ^ 16, ^ 8, ^ 4, ^ 2, ^ 1. The deviations (each d*d rounded before it
       is added) go the same way. It depends on nothing but the inputs; no floating-point atomic anywhere: the same
       bits on every call. (Integer atomics count the corners of a cell; a count has no order.)
   _create() evaluates x at the problem's state and keeps mean, stdev and count of every camera on the device; the
   problem may be destroyed afterwards. Refused: a problem without board observations (only they are binned: point
   observations and regularization are ignored), a problem that is a shard, a grid dimension < 2, more than 2^20 cells
   in all. _grid(): camera icam's grid. _get(): its arrays, [gridn_height][gridn_width], any of them NULL to skip.
   _binning_ms(): the device time of _create()'s launches */
typedef struct mrcal_amd_regional_statistics mrcal_amd_regional_statistics_t;
mrcal_amd_regional_statistics_t* mrcal_amd_regional_statistics_create(mrcal_amd_problem_t* problem, int gridn_width, int gridn_height);
bool   mrcal_amd_regional_statistics_grid(const mrcal_amd_regional_statistics_t* s, int icam_intrinsics, int* gridn_width, int* gridn_height);
bool   mrcal_amd_regional_statistics_get(const mrcal_amd_regional_statistics_t* s, int icam_intrinsics,
                                         double* mean, double* stdev, int32_t* count);
double mrcal_amd_regional_statistics_binning_ms(const mrcal_amd_regional_statistics_t* s);
void   mrcal_amd_regional_statistics_destroy(mrcal_amd_regional_statistics_t* s);

/* ---- valid-intrinsics region: making one from a solve, and applying one ----
   Making (mrcal/calibration.py:1611-1717, _compute_valid_intrinsics_region()). _mask(): on the device, the grid of
   sample_imager() (the centres above) is unprojected through (lensmodel, intrinsics) to unit vectors, multiplied by
   distance (distance <= 0: left as they are, and evaluated at infinity), given to the uncertainty context for the
   worst-direction standard deviation; then, a cell a lane: an uncertainty that is not finite counts as 1e9;
   mask = uncertainty < threshold_uncertainty, and unless the lens model is LENSMODEL_SPLINED_*, also mean <
   threshold_mean (signed, as the reference's code has it), stdev < threshold_stdev, count > threshold_count, from the
   regional statistics of camera icam_intrinsics, which must be on the same grid (s may be NULL for a splined model).
   mask [gridn_height][gridn_width] bytes is what crosses to the host, and the uncertainties as evaluate() gives them
   if uncertainty is not NULL.

   The outline of a mask, _region_outline() (host code, csrc/region_outline.cpp). cv2 is no part of this project; this
   is the definition, and no equality with cv2.findContours() is claimed:
     - the set cells fall into 8-connected components
     - the outline of a component is its outer border, followed from cell centre to cell centre beginning at its
       topmost cell, the leftmost of that row, clockwise on the screen (x to the right, y down): with the 8 directions
       numbered clockwise from east, a cell entered by direction d looks at its neighbours clockwise beginning at
       d + 5 (one past the way back) and goes to the first that is set; the first cell begins looking at east. The
       walk ends when it stands on the first cell about to repeat its first move. A hole has no part in it
     - a spur one cell wide is walked out and back; a component of one cell is that one cell
     - only the cells where the direction changes are kept, as (x,y) = (column, row); the first vertex is not repeated
     - the area of a component is the shoelace area of these vertices; the component with the largest area is the one
       reported, the first in raster order (of the components' first cells) among equals. A line of cells, and a
       single cell, have area 0 and fewer than 3 vertices: closed they have fewer than 4 points, an empty region
   It returns the number of vertices and writes the first min(count, capacity) of them; -1: bad arguments.

   Applying (mrcal/model_analysis.py:2106-2149, is_within_valid_intrinsics_region()). vertices [Nvertices][2] is a
   closed contour (the last vertex repeats the first), the edges join consecutive vertices. A point is inside by the
   even-odd rule, STRICTLY inside: a point on an edge or on a vertex is outside, as with shapely's contains(). A lane
   a point; up to _lds_vertices() = 4096 vertices are held in LDS, a contour with more is read from global memory by
   the same code. With integer vertices and integer-valued points (pixel centres), all below 2^24 in size, the
   decision is exact: every product is an integer a double holds. For other points the decision within rounding of
   an edge is not specified. No vertices: every point is outside. _contains(): N points q [N][2] of the host.
   _image(): every pixel centre of a W x H image in one launch, out [H][W] */
bool mrcal_amd_valid_region_mask(mrcal_amd_uncertainty_t* u, const mrcal_amd_regional_statistics_t* s, int icam_intrinsics,
                                 const mrcal_lensmodel_t* lensmodel, const double* intrinsics, int W, int H,
                                 int gridn_width, int gridn_height, double distance,
                                 double threshold_uncertainty, double threshold_mean, double threshold_stdev, double threshold_count,
                                 uint8_t* mask, double* uncertainty);
int  mrcal_amd_region_outline(const uint8_t* mask, int gridn_width, int gridn_height, int32_t* vertices, int capacity, int64_t* area2);
int  mrcal_amd_valid_region_lds_vertices(void);
bool mrcal_amd_valid_region_contains(uint8_t* out, const double* q, int64_t N, const double* vertices, int Nvertices);
bool mrcal_amd_valid_region_image(uint8_t* out, int W, int H, const double* vertices, int Nvertices);

#ifdef __cplusplus
}
#endif
