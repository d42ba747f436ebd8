/*
 * rt_api.h — C ABI of the MI355X-native path-tracing hot path.
 *
 * This is the drop-in boundary that replaces the reference's CUDA entry
 * points for the per-pixel hot path (primary ray -> BVH traversal ->
 * sphere/quad/AABB intersection -> material scatter -> texture eval ->
 * multi-sample accumulation).  Everything here is plain C: fixed-width
 * integers, doubles and pointers, no C++ or torch types.
 *
 * Reference interfaces replaced (paths relative to the reference repo):
 *   rt_camera_setup   <- Camera::initialize             src/core/camera/Camera.cpp:31-73
 *   rt_scene_create   <- initialize_cuda_scene          src/scene/CudaSceneInitialization.cuh:249-300
 *                        (+ HittableConverter::cpu_to_cuda_hittable, HittableConverter.cuh:50-111,
 *                           MaterialConverter.cuh:26-121, TextureConverter.cuh:19-88,
 *                           CudaSceneContext::initialize/finalize_and_upload, CudaSceneContext.cuh:71-123)
 *   rt_scene_create_tuned <- the same with the launch / staging / builder tuning passed
 *                        explicitly (rt_tuning; the reference's CameraConfig,
 *                        src/core/camera/CameraConfig.hpp:9-62, carries its settings the same way)
 *   rt_scene_destroy  <- cleanup_cuda_scene             src/scene/CudaSceneInitialization.cuh:302-308
 *   rt_render         <- cuda_init_rand_states_wrapper  src/core/camera/CameraKernelWrappers.cuh:11-13
 *                        + cuda_static_render_wrapper   src/core/camera/CameraKernelWrappers.cuh:25-34
 *                        + the per-batch memset/sync/D2H copy of StaticCamera::render_gpu
 *                                                       src/core/camera/StaticCamera.cpp:235-300
 *   rt_render_device  <- same, but accumulating raw sample sums into a caller-owned device
 *                        buffer on a caller stream (multi-GPU sample sharding / progressive
 *                        accumulation; the role of dynamic_render_tile_kernel's accumulation
 *                        buffer, CameraKernels.cu:206-236)
 *   rt_multi_create / rt_multi_render / rt_multi_destroy
 *                     <- StaticCamera::render_gpu's single-device batch loop
 *                        (src/core/camera/StaticCamera.cpp:136-313) extended to N devices:
 *                        one scene and one host thread per shard, 8x8 tiles dealt
 *                        round-robin over the shards (SURVEY §8(b) "Threading")
 *   rt_tiles_sum_device / rt_tiles_to_frame_device
 *                     <- the batch assembly of StaticCamera::render_gpu (the D2H copy of each
 *                        64-row batch into its rows of the frame, StaticCamera.cpp:281-299) for
 *                        tile shards: chunk partials summed and tiles reordered into frame rows
 *                        on the device, before the one copy out
 *   rt_render_tiles_device / rt_adaptive_update_device / rt_adaptive_select_device /
 *   rt_to_bytes_tiles_device
 *                     <- no counterpart: DynamicCamera traces every stratum of every pixel
 *                        (DynamicCamera.cpp:96-200); these stop sampling the 8x8 tiles whose
 *                        estimate has converged (launches over a tile list, per-pixel moments,
 *                        per-tile error, a display scale per tile)
 *   rt_render_guides_device / rt_denoise_workspace_bytes / rt_denoise_device
 *                     <- no counterpart: DynamicCamera displays the raw accumulation
 *                        (DynamicCamera.cpp:284-300); these give the display first-hit
 *                        albedo / normal / depth sums and an edge-avoiding filter over them
 *   rt_denoise_variance_workspace_bytes / rt_denoise_variance_device
 *                     <- no counterpart: the same filter steered by the variance of each pixel's
 *                        estimate (the adaptive sampler's moments, or a spatial estimate), so
 *                        that it narrows as the frame converges
 *   rt_history_bytes / rt_temporal_device
 *                     <- no counterpart: DynamicCamera clears its accumulation when the camera
 *                        moves (DynamicCamera.cpp:269-276); these reproject the previous pose's
 *                        displayed image into the new pose and blend it with the new samples
 *   rt_scene_move_spheres / rt_scene_move_spheres_device / rt_multi_move_spheres
 *                     <- no counterpart: the reference converts and uploads its scene once
 *                        (CudaSceneInitialization.cuh:249-300) and DynamicCamera moves only the
 *                        camera; these move world spheres of a live scene and refit the world
 *                        BVH's boxes on the device
 *   rt_scene_set_transforms / rt_scene_move_quads (and their _device / rt_multi_ forms),
 *   rt_rotate_y_sincos
 *                     <- no counterpart, as above: these set translate / rotate_y objects and
 *                        move quads of a live scene; media boxes and the world BVH follow
 *   rt_scene_pose_device / rt_motion_device / rt_temporal_motion_device /
 *   rt_temporal_variance_motion_device
 *                     <- no counterpart, as above: per pixel, where the surface under it stood
 *                        before those edits, and the reprojection read there, so that a moved
 *                        object does not cost the display its history
 *   rt_last_error     <- replaces CUDA_CHECK's exit() and the converters' exceptions
 *                        (CudaMemoryUtility.cuh:9-15, HittableConverter.cuh:103-108): errors are
 *                        returned as negative codes, never thrown or exit()ed across the ABI.
 *
 * Scene description.  The reference hands the GPU a pointer graph built from
 * shared_ptr<Hittable> objects.  Here the caller serialises that graph into
 * flat tables (textures, Perlin tables, materials, objects, child lists) whose
 * entries mirror the reference classes one to one; rt_scene_create copies them,
 * builds its own acceleration structure and uploads a device layout that the
 * library owns.  The caller owns every pointer it passes in.
 *
 * Threading.  Distinct rt_scene objects are independent and may be used from
 * different host threads (and devices) at once.  One rt_scene is used by one
 * host thread at a time: its kernel-timing events, its scratch / staging
 * buffers, its work-unit counter (persistent launches) and its tile-cost /
 * dispatch-order buffers (rt_tuning.no_tile_order) are per scene.
 * A scene's launches run one after another even on different caller streams:
 * each launch waits for the scene's previous one (an event), since they share
 * the scene's work-unit counter, scratch and tile orders; the caller orders
 * its own buffers' producers and consumers with its streams as for any device
 * work.  Destroying a scene, or a launch that grows its buffers, waits for
 * that scene's own work only -- its stream and its last launch -- never for
 * other scenes' or threads' work on the device: scene memory comes from a
 * library-owned pool per device (hipMallocFromPoolAsync on the scene's
 * stream) because a plain hipFree waits for the whole device, and destroy
 * queues nothing on any stream (a stream may share a hardware queue with a
 * busy one): a destroyed scene's idle buffers are freed by the next
 * allocation on the device, or at process exit.  Tile orders are kept per
 * launch shape (four shapes per scene, least recently used replaced).
 *
 * Numerics.  All arithmetic is fp64, as in the reference (Vec3.hpp:184).  The
 * random stream is a stateless counter-based Philox4x32-10 keyed by
 * (seed, pixel, stratum sample, bounce, slot); see DESIGN.md "RNG contract".
 */
#ifndef RT_API_H
#define RT_API_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever a struct layout or a signature below changes.  A caller
   checks rt_abi_version() == the RT_ABI_VERSION it was compiled against before
   any other call (rtx/lib.py does): structs are passed by pointer without a
   size field, so a caller built against another version must not proceed.
   2: rt_scene_desc.bvh_arity, rt_path_stats.cyc_*, rt_scene_info's stack and
      LDS fields.
   3: rt_tiles_sum_device, rt_tiles_to_frame_device, rt_multi_gather_ms; the
      rt_multi exchange runs on the devices.
   4: rt_tuning with rt_scene_create_tuned / rt_multi_create_tuned (the
      library reads no environment variables); rt_path_stats.medium_box_*;
      rt_scene_info.lds_node_bytes.
   5: strata_chunks = RT_CHUNKS_AUTO (rt_render_device, RT_LAYOUT_TILES): the
      library's work units for a tile subset, per-tile sums out; rt_tuning
      sub_* and no_tile_order fields (in four of the reserved slots: same size
      and offsets); round 6: rt_tuning.probe_strata (a fifth reserved slot,
      zero = the default, so version 5 callers are unaffected). */
#define RT_ABI_VERSION 5

/* ---- status codes ------------------------------------------------------ */
#define RT_OK 0
#define RT_ERR_INVALID (-1)     /* malformed description / argument */
#define RT_ERR_DEVICE (-2)      /* HIP runtime error (message in rt_last_error) */
#define RT_ERR_OOM (-3)         /* device allocation failed */
#define RT_ERR_UNSUPPORTED (-4) /* valid but not supported (e.g. nesting too deep) */

typedef struct rt_vec3 {
  double x, y, z;
} rt_vec3;

/* ---- textures (Texture.hpp:8-18) ---------------------------------------- */
enum {
  RT_TEX_SOLID = 0,   /* SolidColorTexture   SolidColorTexture.cpp:8-10 */
  RT_TEX_CHECKER = 1, /* CheckerTexture      CheckerTexture.cpp:41-55   */
  RT_TEX_NOISE = 2    /* NoiseTexture        NoiseTexture.cpp:31-34     */
};

typedef struct rt_texture_desc {
  int32_t kind;
  int32_t even;   /* checker: texture index used when the cell parity is even */
  int32_t odd;    /* checker: texture index used when the parity is odd */
  int32_t perlin; /* noise: index into rt_scene_desc.perlin */
  double scale;   /* checker cell size / noise frequency */
  rt_vec3 color;  /* solid colour */
} rt_texture_desc;

/* Perlin gradient + permutation tables (PerlinNoise.hpp:19-33, 150-160). */
#define RT_PERLIN_POINTS 256
typedef struct rt_perlin_desc {
  rt_vec3 rand_vec[RT_PERLIN_POINTS];
  int32_t perm_x[RT_PERLIN_POINTS];
  int32_t perm_y[RT_PERLIN_POINTS];
  int32_t perm_z[RT_PERLIN_POINTS];
} rt_perlin_desc;

/* ---- materials (Material.hpp:11-46) ------------------------------------- */
enum {
  RT_MAT_LAMBERTIAN = 0,    /* LambertianMaterial.cpp:15-59   */
  RT_MAT_METAL = 1,         /* MetalMaterial.cpp:43-62        */
  RT_MAT_DIELECTRIC = 2,    /* DielectricMaterial.cpp:58-85   */
  RT_MAT_DIFFUSE_LIGHT = 3, /* DiffuseLightMaterial.cpp:12-22 */
  RT_MAT_ISOTROPIC = 4      /* IsotropicMaterial.cpp:12-31    */
};

typedef struct rt_material_desc {
  int32_t kind;
  int32_t texture;         /* lambertian / diffuse_light / isotropic */
  rt_vec3 albedo;          /* metal */
  double fuzz;             /* metal */
  double refraction_index; /* dielectric */
} rt_material_desc;

/* ---- hittables (Hittable.hpp:12-50) -------------------------------------- */
enum {
  RT_OBJ_SPHERE = 0,    /* Sphere (static / moving)   Sphere.cpp:8-28, 101-178 */
  RT_OBJ_QUAD = 1,      /* Plane == parallelogram     Plane.cpp:6-132          */
  RT_OBJ_LIST = 2,      /* HittableList               HittableList.cpp:26-63   */
  RT_OBJ_ROTATE_Y = 3,  /* RotateY                    RotateY.cpp:5-103        */
  RT_OBJ_TRANSLATE = 4, /* Translate                  Translate.cpp:7-39       */
  RT_OBJ_MEDIUM = 5     /* ConstantMedium             ConstantMedium.cpp:25-94 */
};

#define RT_STORED_FORM 2

typedef struct rt_object_desc {
  int32_t kind;
  int32_t material; /* sphere / quad: material index, -1 = none (light-list entries) */
  int32_t child;    /* rotate_y / translate / medium: object index of the wrapped object;
                       list: first index into rt_scene_desc.children */
  int32_t count;    /* list: number of children */
  rt_vec3 a;        /* sphere: centre (t=0);  quad: corner Q;  translate: offset */
  rt_vec3 b;        /* sphere: centre at t=1 (moving only);  quad: side u */
  rt_vec3 c;        /* quad: side v */
  double s;         /* sphere: radius;  rotate_y: angle in degrees;  medium: density */
  int32_t moving;   /* sphere: 0 static; 1 = two-centre constructor, b = centre at t=1
                       (Sphere.cpp:15-23); RT_STORED_FORM = b is the stored displacement
                       c1 - c0 (Sphere::get_center().direction()).
                       rotate_y: RT_STORED_FORM = (a.x, a.y) are the stored (sin, cos)
                       (RotateY.hpp m_sin_theta/m_cos_theta) instead of s degrees.
                       The stored forms let a binding hand over the reference objects'
                       own doubles without a lossy round trip. */
  int32_t phase;    /* medium: material index of the phase function (isotropic) */
} rt_object_desc;

typedef struct rt_scene_desc {
  const rt_texture_desc *textures;
  int32_t n_textures;
  int32_t n_perlin;
  const rt_perlin_desc *perlin;
  const rt_material_desc *materials;
  int32_t n_materials;
  int32_t n_objects;
  const rt_object_desc *objects;
  const int32_t *children; /* list child tables */
  int32_t n_children;
  int32_t world;   /* object index of the world list (main.cpp:142 `HittableList world`) */
  int32_t lights;  /* object index of the lights list, -1 = no lights */
  int32_t use_bvh; /* reference -b: lights become HittableList(BVHNode(lights))
                      (StaticCamera.cpp:35-40); the world is always traversed through
                      the library's own BVH (closest hit is structure independent) */
  int32_t bvh_builder; /* RT_BVH_AUTO (0): device binned SAH from 65536 world
                          primitives, host SAH below; RT_BVH_HOST; RT_BVH_DEVICE
                          (linear BVH); RT_BVH_DEVICE_SAH */
  int32_t bvh_arity;   /* world BVH node width: 0 = auto (4 from 4096 world
                          primitives, else 2), 2, or 4 (the binary tree collapsed
                          to 4-wide nodes) */
} rt_scene_desc;

enum {
  RT_BVH_AUTO = 0,
  RT_BVH_HOST = 1,  /* binned SAH on the host (rt_scene.cpp) */
  RT_BVH_DEVICE = 2, /* linear BVH on the GPU (rt_bvh_build.hip) */
  RT_BVH_DEVICE_SAH = 3 /* binned SAH on the GPU, level by level (rt_bvh_sah.hip) */
};

/* ---- camera (CameraConfig.hpp:9-35) ------------------------------------- */
typedef struct rt_camera_desc {
  int32_t image_width;
  int32_t samples_per_pixel;
  int32_t max_depth;
  int32_t _pad0;
  double aspect_ratio;
  double vfov;
  double defocus_angle;
  double focus_dist;
  rt_vec3 lookfrom;
  rt_vec3 lookat;
  rt_vec3 vup;
  rt_vec3 background;
} rt_camera_desc;

/* The camera frame Camera::initialize derives (Camera.hpp:110-141 members);
   exactly the arguments cuda_static_render_wrapper takes. */
typedef struct rt_frame {
  int32_t image_width;
  int32_t image_height;
  int32_t sqrt_spp; /* int(sqrt(samples_per_pixel)) (StaticCamera.cpp:74-76) */
  int32_t max_depth;
  rt_vec3 center;
  rt_vec3 pixel00_loc;
  rt_vec3 pixel_delta_u;
  rt_vec3 pixel_delta_v;
  rt_vec3 u, v, w;
  rt_vec3 defocus_disk_u;
  rt_vec3 defocus_disk_v;
  double defocus_angle;
  double pixel_samples_scale; /* 1/samples_per_pixel (Camera.cpp:35) */
  rt_vec3 background;
} rt_frame;

/* ---- render ---------------------------------------------------------------- */
enum {
  RT_OUT_SCALED = 0, /* out = pixel_samples_scale * sum (StaticCamera.cpp:98) */
  RT_OUT_SUM = 1     /* out = raw sum over the launched samples */
};

enum {
  RT_LAYOUT_FRAME = 0,
  RT_LAYOUT_TILES = 1
};

typedef struct rt_render_params {
  int32_t row_begin;    /* first image row (inclusive) — StaticCamera.cpp:235 batches */
  int32_t row_end;      /* last row (exclusive); 0,0 = whole image */
  int32_t sample_begin; /* first linear stratum index s_j*sqrt_spp+s_i */
  int32_t sample_count; /* number of strata; -1 = all sqrt_spp^2 */
  uint64_t seed;        /* RNG key; replaces curand_init(time(nullptr)+pixel) */
  int32_t output;       /* RT_OUT_SCALED / RT_OUT_SUM */
  int32_t accumulate;   /* rt_render_device only: 1 = add into the buffer, 0 = overwrite */
  /* Tile subset (multi-GPU tile sharding): the 8x8 tiles of the row range, in
     row-major tile order, are rendered for t = tile_first + k*tile_stride only.
     tile_stride 0 or 1 with tile_first 0 = every tile. */
  int32_t tile_first;
  int32_t tile_stride;
  int32_t layout;       /* RT_LAYOUT_FRAME: row-major pixels (index (j-row_begin)*W+i);
                           RT_LAYOUT_TILES: the k-th rendered tile's 64 pixels at
                           [k*64, k*64+64), pixel (x,y) of the tile at k*64 + y*8 + x
                           (slots outside the image hold 0) */
  int32_t strata_chunks; /* RT_LAYOUT_TILES only: split each tile's strata into this
                            many equal consecutive chunks, each traced by its own
                            wavefront (finer work units for small tile subsets);
                            the output becomes [tile k][chunk c][64 px][3], whose
                            chunk sums are the tile's sums.  0 or 1 = one chunk.
                            RT_CHUNKS_AUTO (rt_render_device only, with RT_OUT_SUM
                            and accumulate 0): the library splits the subset into
                            work units sized to the device (a head/tail plan: the
                            last tiles in finer chunks, taken last) and returns
                            the per-tile sums [tile k][64 px][3], the chunk
                            partials added on the device in chunk order on the
                            same stream. */
} rt_render_params;
#define RT_CHUNKS_AUTO (-1)

/* Per-launch traversal/shading counters (for algorithmic-bytes accounting). */
typedef struct rt_path_stats {
  uint64_t samples;        /* camera samples traced */
  uint64_t segments;       /* ray segments (world traversals) */
  uint64_t node_visits;    /* BVH node fetches */
  uint64_t sphere_tests;   /* ray-sphere intersection tests (world traversal) */
  uint64_t quad_tests;     /* ray-quad tests (world traversal) */
  uint64_t other_tests;    /* instance / medium / list object visits */
  uint64_t light_tests;    /* primitive tests done by light pdf_value */
  uint64_t shade_events;   /* material evaluations */
  /* SIMD efficiency: iterations summed over wavefronts (each iteration occupies
     64 lane slots; e.g. node_visits / (64 * wave_node_iters) is the fraction of
     lanes doing useful node work) */
  uint64_t wave_trips;      /* path-loop trips (one segment attempt per lane) */
  uint64_t wave_node_iters; /* traversal node-loop iterations */
  uint64_t wave_leaf_iters; /* leaf-item loop iterations */
  uint64_t wave_shade_iters; /* shading branch executions (lambertian/metal/dielectric/light) */
  /* Where a wavefront's time goes: shader cycles (s_memtime) summed over
     wavefronts, each region counted once per wave visit -- the loop overall,
     camera-ray regeneration, closest-hit queries (traversal + items + media +
     record), the media part of them, material shading, light sampling + light
     pdf, texture evaluation.  Instrumentation adds a few percent; the shares
     are what matters. */
  uint64_t cyc_loop, cyc_regen, cyc_trace, cyc_media, cyc_shade, cyc_lights;
  /* Traversal-SIMD model (summed over wavefronts): model_trace_max = the sum
     over path trips of the largest per-lane node-visit count of the trip (the
     node-loop iterations a wave needs with one walk per lane);
     model_trace_pair_max = the same with each lane's walks of two consecutive
     trips run back to back in one node loop (max over lanes of the pair's
     sum) -- what two walks per lane could at best save. */
  uint64_t model_trace_max, model_trace_pair_max;
  /* Noise-texture albedo evaluations (shading events whose texture is a
     NoiseTexture): lanes, and wavefront executions of that evaluation (their
     ratio / 64 is the evaluation's lane use). */
  uint64_t noise_evals, wave_noise_iters;
  /* Constant media with a box boundary (make_box): lanes whose boundary
     queries took the six-face slab form, and lanes of those it deferred to
     the general boundary scan (edge / corner / parallel rays within its
     margin; ABI 4). */
  uint64_t medium_box_tests, medium_box_deferred;
} rt_path_stats;

typedef struct rt_scene_info {
  int32_t n_nodes;     /* world BVH nodes */
  int32_t n_leaf_refs; /* object references in BVH leaves */
  int32_t n_spheres, n_quads, n_objects, n_light_leaves;
  int32_t bvh_depth;
  int32_t node_bytes;   /* bytes per BVH node in the device layout */
  int32_t sphere_bytes; /* bytes per sphere record */
  int32_t quad_bytes;   /* bytes per quad record */
  int64_t device_bytes; /* total device bytes of the scene */
  int32_t features;     /* kernel instance: bit0 media, bit1 transforms, bit2 lights, bit3 noise,
                           bit4 flat world, bit5 4-wide BVH; bit6: every material is Lambertian
                           with a solid colour (a world of bit4 alone then runs the
                           Lambertian-only instance) */
  int32_t lds_nodes;    /* BVH nodes (BFS prefix) the kernel stages in LDS per block */
  int32_t bvh_builder;  /* the builder that made the world BVH: RT_BVH_HOST / RT_BVH_DEVICE /
                           RT_BVH_DEVICE_SAH */
  int32_t bvh_arity;    /* 2 or 4 (n_nodes, lds_nodes and node_bytes count nodes of this width) */
  int32_t stack_depth;  /* traversal stack entries per lane (1 + BVH levels; 3 per 4-wide level) */
  int32_t lds_fixed_bytes;  /* LDS per block the kernel needs before staging nodes: static
                               accumulators + traversal stacks of its 4 wavefronts */
  int32_t lds_block_budget; /* LDS per block at the kernel's occupancy target; the node prefix
                               fills what lds_fixed_bytes leaves (LDS never lowers occupancy) */
  int32_t waves_per_simd;   /* occupancy target of the kernel instance the scene selects */
  int32_t lds_nodes_persistent; /* BVH nodes staged by the persistent frame instance (one
                                   16-wave block per CU owning its 160 KB of LDS); -1: the
                                   scene's frames run one work unit per wavefront */
  int32_t lds_prims_persistent; /* 1: the persistent frame instance also stages every world
                                   item and sphere in LDS (whole tree staged and room left) */
  int32_t persistent_block_waves; /* waves per block of the persistent instance: 16 (one block
                                     per CU) or 4 (traversal stacks too deep for 16); 0: none */
  int32_t lds_perlin; /* 1: the scene's Perlin table (one noise texture source) is staged in
                         LDS by every block of the noise instances; 0: read from HBM */
  int32_t lds_node_bytes; /* bytes per BVH node as staged in LDS (DNodeL 80 / DNode4 128;
                             node_bytes is the HBM layout's, ABI 4) */
} rt_scene_info;

typedef struct rt_scene rt_scene; /* opaque, library-owned */

int rt_abi_version(void);
const char *rt_last_error(void); /* thread-local; valid until the next call */
int rt_device_count(int32_t *count);

int rt_camera_setup(const rt_camera_desc *camera, rt_frame *frame);

/* Tuning of one scene's launches, passed explicitly at creation instead of
   read from the process environment (the reference passes its configuration
   the same way, CameraConfig.hpp:9-62).  A zero-filled struct is the default
   plan of every field -- what rt_scene_create uses.  None of the fields
   changes a rendered value: the frame is the same sum of the same samples,
   only its split into work units, the LDS staging and the BVH builder's
   parameters move (work-unit splits regroup a pixel's fp64 chunk sums, so
   frames of different splits agree to rounding, not bit for bit). */
typedef struct rt_tuning {
  /* frame work units (rt_render*, rt_multi_render) */
  int32_t chunk_target;   /* uniform split: work units per wave slot; 0: 32; < 0: whole tiles only */
  int32_t head_strata;    /* head/tail plan: strata per head unit; 0: 64 up to 64 strata, else 128 */
  int32_t tail_split;     /* tail chunks per head chunk; 0: 8 */
  int32_t no_uniform_tail; /* 1: no finer last chunks in the uniform split */
  int32_t no_persistent;  /* 1: one work unit per wavefront (no persistent unit loop) */
  int32_t grid_cap;       /* persistent launches: at most this many blocks; 0: every resident one */
  double tail_tiles;      /* tail tiles per wave slot; 0: 0.25 (head/tail plan), 0.5 (after the
                             uniform split); < 0: no tail plan */
  /* LDS staging (rt_scene_create) */
  int32_t lds_nodes;      /* one-unit instances: at most this many BVH nodes; 0: the plan; < 0: none */
  int32_t lds_nodes_pc;   /* the persistent instance's node prefix, the same rule */
  int32_t no_lds_prims;   /* 1: the persistent instance stages no items / spheres */
  int32_t no_lds_perlin;  /* 1: the Perlin table stays in HBM */
  int32_t lds_cap;        /* per-block LDS cap in bytes; 0: 64 KB (tests of the stack fallback) */
  int32_t pc_waves;       /* persistent blocks: 0 auto; 4: the 4-wave form on any scene (tests) */
  /* world BVH builders */
  int32_t sah_stack_budget; /* device SAH: depth of the balanced-split switch; 0: RT_STACK_DEPTH-2 */
  int32_t lbvh_max_depth;   /* device trees deeper than this fall back to the host SAH; 0: RT_STACK_DEPTH-1 */
  int32_t sah_leaf_max, sah_leaf_split; /* host SAH leaf rules; 0: the builder's defaults */
  int32_t sah_trav_x4, sah_bins;        /* host SAH traversal cost x4, bins; 0: 4, 16 */
  int32_t extra_features;   /* RT_FEAT_* bits OR'ed into the kernel instance key (debug) */
  /* tile-subset work units (rt_render_device, strata_chunks = RT_CHUNKS_AUTO);
     subsets of more than 4 tiles per wave slot take the frame plan above */
  int32_t sub_head_strata;   /* strata per head unit; 0: 16 x sqrt(strata / 64) */
  int32_t sub_tail_split;    /* tail chunks per head chunk; 0: 2 */
  int32_t sub_tail_permille; /* tail tiles per 1000 wave slots; 0: 125; < 0: none */
  int32_t no_tile_order;     /* 1: launches take their tiles in plan order (default: a probe launch
                                measures the tile costs once per launch shape and the launches of
                                the shape take them most expensive first; the frames are the
                                same bit for bit) */
  int32_t probe_strata;      /* strata per pixel of the probe launch that measures a launch shape's
                                tile costs for its dispatch order, once per shape; 0: 16 */
  int32_t reserved[2];
} rt_tuning;

int rt_scene_create(const rt_scene_desc *desc, int32_t device, rt_scene **scene);
/* rt_scene_create with explicit tuning (NULL: the default, as rt_scene_create) */
int rt_scene_create_tuned(const rt_scene_desc *desc, int32_t device, const rt_tuning *tuning,
                          rt_scene **scene);
int rt_scene_info_get(const rt_scene *scene, rt_scene_info *info);
/* Waits for the scene's own pending work (rt_render_device launches on any
   caller stream included), then releases it; NULL is a no-op. */
int rt_scene_destroy(rt_scene *scene);

/* Render rows [row_begin,row_end) x strata [sample_begin, +sample_count) and
   copy to host_rgb (row-major, 3 doubles per pixel, index (j-row_begin)*W+i).
   Synchronous, like the reference's per-batch loop. */
int rt_render(rt_scene *scene, const rt_frame *frame, const rt_render_params *params,
              double *host_rgb);

/* Same work, asynchronously on `hip_stream` (NULL = the HIP null stream, so work
   is ordered with a framework's default stream, e.g. torch's),
   writing/accumulating into a device buffer of W*(row_end-row_begin)*3 doubles. */
int rt_render_device(rt_scene *scene, const rt_frame *frame,
                     const rt_render_params *params, double *device_rgb,
                     void *hip_stream);

/* SAH cost of the world BVH, relative to the root box: 1 (the root) + the sum
   over every node's two children of area(child) / area(root) x (leaf: its item
   count; inner: 1) -- the tree-quality figure of the reference's builder
   (BVHNode.cpp:215-254, unit traversal and intersection costs).  0 for a flat
   world.  Always the BINARY tree the builder made (for a 4-wide scene, the
   tree before the collapse, costed at creation); otherwise copies the nodes
   back from the device.  After rt_scene_move_spheres* a binary scene therefore
   reports the refitted tree -- the caller's signal for when a rebuild
   (rt_scene_rebuild_bvh) pays -- while a 4-wide scene keeps returning the
   figure of the binary tree it was last collapsed from, which is not kept:
   creation's, and after rt_scene_rebuild_bvh the rebuilt binary tree's. */
int rt_scene_bvh_cost(const rt_scene *scene, double *cost);

/* Run the counter-instrumented kernel variant (untimed) and return totals. */
int rt_render_stats(rt_scene *scene, const rt_frame *frame,
                    const rt_render_params *params, rt_path_stats *stats);

/* Device time of the last render kernel launched on this scene, measured with
   HIP events recorded on the launch stream around the kernel (ms). */
int rt_last_kernel_ms(rt_scene *scene, double *ms);

/* Quantise a device radiance buffer to 8-bit RGB on the device with the
   reference's write_color rule (ColorUtility.hpp:11-36). */
int rt_to_bytes_device(const double *device_rgb, int64_t n_pixels, double scale,
                       uint8_t *device_bytes, void *hip_stream);

/* ---- adaptive sampling (functions added under ABI 5: no struct or signature
   above changed) ------------------------------------------------------------
   Progressive accumulation that stops sampling the 8x8 tiles whose estimate
   has converged (rtx/adaptive.py drives these; DESIGN.md "Adaptive sampling").
   Tiles are numbered row-major over the row range / the frame, as
   tile_first / tile_stride number them.  A tile list is device resident,
   strictly ascending and in range -- the caller's contract; every entry is
   clamped into [0, tiles - 1] on the device before use, so a bad list can
   mis-render but never reaches memory outside the buffers described. */

/* rt_render_device in RT_LAYOUT_FRAME restricted to the n_tiles tiles of
   device_tiles: only their pixels are written (accumulate 0) or added to
   (accumulate 1), every other pixel of device_rgb is left untouched.
   params->tile_first / tile_stride / layout / strata_chunks must be
   0 / 0-or-1 / RT_LAYOUT_FRAME / 0.  n_tiles 0 queues nothing; n_tiles above
   the range's tile count is RT_ERR_INVALID.  The list is copied (a kernel on
   hip_stream) into a scene-owned buffer, so work queued on hip_stream after
   the call may rewrite it.  One stratum per launch gives each listed
   pixel the value rt_render_device gives it bit for bit; more strata may be
   split into other work units than the full frame's (rt_tuning's caveat:
   agreement to rounding).  No dispatch order is measured or kept for a list. */
int rt_render_tiles_device(rt_scene *scene, const rt_frame *frame, const rt_render_params *params,
                           const int32_t *device_tiles, int32_t n_tiles, double *device_rgb,
                           void *hip_stream);

/* One batch of batch_strata strata per pixel, rendered as raw sums into
   device_delta ([H][W][3]), folded into the state of the listed tiles -- one
   wavefront per tile, one lane per pixel.  Per pixel: acc += delta; with
   y = (0.2126 r + 0.7152 g + 0.0722 b of delta) / batch_strata: s1 += y,
   s2 += y * y (s1, s2: [H][W]).  Per tile: tile_strata[t] += batch_strata
   (tile_strata: [tiles of the frame]). */
int rt_adaptive_update_device(const double *device_delta, int32_t batch_strata, const int32_t *device_tiles,
                              int32_t n_tiles, const rt_frame *frame, double *device_acc, double *device_s1,
                              double *device_s2, int32_t *device_tile_strata, void *hip_stream);

/* The tiles of device_tiles_in that still need samples, in the same
   (ascending) order, into device_tiles_out (room for n_in entries; must not
   alias the input), their number into device_count_out[0].  For a tile with
   b = tile_strata[t] / batch_strata batches, per pixel inside the image:
   mean = s1 / b, var = max(0, (s2 - s1 * s1 / b) / (b - 1)),
   se = sqrt(var / b); the tile's error e_t is the average of
   se / (mean + floor) over those pixels (infinite while b < 2), stored in
   device_tile_error[t] unless that is NULL.  A tile is dropped when
   b >= max(2, min_batches) and e_t <= threshold.  Flags and a scan, no
   atomics: the output is reproducible. */
int rt_adaptive_select_device(const double *device_s1, const double *device_s2,
                              const int32_t *device_tile_strata, int32_t batch_strata, const rt_frame *frame,
                              double threshold, double floor, int32_t min_batches,
                              const int32_t *device_tiles_in, int32_t n_in, int32_t *device_tiles_out,
                              int32_t *device_count_out, double *device_tile_error, void *hip_stream);

/* rt_to_bytes_device over a frame ([H][W][3]) with the scale
   1 / max(1, tile_strata[tile of the pixel]) per pixel. */
int rt_to_bytes_tiles_device(const double *device_rgb, const int32_t *device_tile_strata, const rt_frame *frame,
                             uint8_t *device_bytes, void *hip_stream);

/* ---- denoised display (functions added under ABI 5: no struct or signature
   above changed) ------------------------------------------------------------
   First-hit guide buffers and an edge-avoiding a-trous filter for the first
   frames after a camera move (rtx/denoise.py drives these and states the
   filter in NumPy; DESIGN.md "Denoised display"). */

/* Per-pixel guide sums: albedo r,g,b; normal x,y,z; depth; hits. */
#define RT_GUIDE_CHANNELS 8

/* Adds (accumulate 1) or writes (0) the first-hit guide sums of strata
   [sample_begin, +sample_count) of rows [row_begin, row_end) into
   device_guides ([rows][W][RT_GUIDE_CHANNELS] doubles), asynchronously on
   hip_stream.  A sample's ray is the render's own camera ray of that stratum
   (same seed, jitter, defocus, time); its first hit is the render's primary
   segment's, constant media included.  Per sample: a miss adds albedo (1,1,1)
   and nothing else; a hit adds hits 1, depth t * |d|, the surface normal
   (0 for a medium) and the albedo -- the texture value (lambertian, a
   medium's isotropic phase), the metal's albedo, or (1,1,1) (dielectric,
   diffuse light).  One wavefront per 8x8 tile, one lane per pixel, strata
   added in ascending order: the result is bit-reproducible, and strata [0,4)
   in one call equal [0,2) then [2,4) accumulated bit for bit.  Pixels outside
   the image are not written.  params->output must be RT_OUT_SUM; tile_first /
   tile_stride / layout / strata_chunks must be 0 / 0-or-1 / RT_LAYOUT_FRAME /
   0; anything else is RT_ERR_INVALID before anything is queued.  The launch
   joins the scene's launch chain like rt_render_device (rt_scene_destroy waits
   for it). */
int rt_render_guides_device(rt_scene *scene, const rt_frame *frame, const rt_render_params *params,
                            double *device_guides, void *hip_stream);

/* The filter's defaults: chosen by the sweep of tools/denoise_bench.py
   (DESIGN.md "Denoised display" records it). */
#define RT_DENOISE_PASSES 5
#define RT_DENOISE_SIGMA_NORMAL 0.2
#define RT_DENOISE_SIGMA_DEPTH 0.01
#define RT_DENOISE_SIGMA_HIT 0.1
#define RT_DENOISE_SIGMA_COLOR 64.0
#define RT_DENOISE_MAX_PASSES 8

typedef struct rt_denoise_params {
  int32_t passes;      /* a-trous passes, step 2^k in pass k; 0: RT_DENOISE_PASSES; < 0: none
                          (prepare + remodulate only); > RT_DENOISE_MAX_PASSES: RT_ERR_INVALID */
  int32_t reserved;
  double sigma_normal; /* 0: default; < 0: term off */
  double sigma_depth;  /* 0: default; < 0: term off */
  double sigma_hit;    /* 0: default; < 0: term off */
  double sigma_color;  /* 0: default; < 0: term off; halves every pass */
} rt_denoise_params;

/* Bytes of workspace rt_denoise_device needs for this frame (a multiple of
   256): four fp32 float4 planes, 64 B per pixel. */
int rt_denoise_workspace_bytes(const rt_frame *frame, int64_t *bytes);

/* out = the a-trous-filtered, scaled radiance of device_rgb, steered by the
   guides.  Per pixel: c = rgb * scale (rgb_scale, or with device_tile_strata
   1 / max(1, strata of the pixel's 8x8 tile) as rt_to_bytes_tiles_device);
   a = albedo / g, a_d = max(a, 0.01) per channel, e = c / a_d (the filtered
   signal); n = normal / g (not renormalised), h = hits / g,
   z = depth / max(hits, 1), all rounded to fp32.  Pass k = 0 .. passes - 1,
   step s = 2^k: taps q = p + s (di, dj), di, dj in -2..2, B3-spline weights
   b = (1/16, 1/4, 3/8, 1/4, 1/16), taps outside the image skipped; the centre
   weighs b2 b2; every other tap b_di b_dj exp(-min(x, 80)) with x the sum of
   the enabled terms |n_p - n_q|^2 / sn^2, |z_p - z_q| / (sz max(z_p, z_q,
   1e-30) s max(|di|, |dj|)), (h_p - h_q)^2 / sh^2 and |e_p - e_q|^2 /
   ((sc 2^-k)^2 (y_p^2 + 1e-4)), y the Rec. 709 luminance of e; a tap whose e
   is not finite weighs 0 (a non-finite e_p has no colour term);
   e'_p = sum w e_q / sum w, or e_p itself when sum w = 0.  out = e a_d.
   device_rgb and the guides are only read; device_out may be device_rgb and
   must not overlap the workspace (256-B aligned, caller-owned: the library
   allocates nothing and keeps no state).  Needs no rt_scene; runs on the
   current device. */
int rt_denoise_device(const rt_frame *frame, const double *device_rgb, double rgb_scale,
                      const int32_t *device_tile_strata, const double *device_guides, int32_t guide_strata,
                      const rt_denoise_params *params, void *device_workspace, double *device_out,
                      void *hip_stream);

/* ---- variance-guided display filter (functions and one struct added under
   ABI 5: no struct or signature above changed) --------------------------------
   rt_denoise_device's colour term is normalised by the pixel's own luminance:
   it blurs a converged frame as much as a noisy one.  This second entry point
   normalises by the standard deviation of the pixel's estimate, so the filter
   narrows as the estimate converges (rtx/denoise.py states it in NumPy,
   NumpyOps.denoise_variance; DESIGN.md "Variance-guided display filter"). */

/* The filter's own defaults: sigma_lum is the best point of the sweep of
   tools/variance_bench.py (DESIGN.md records it); passes, sigma_normal,
   sigma_depth and sigma_hit default to RT_DENOISE_* above. */
#define RT_DENOISE_SIGMA_LUM 4.0
#define RT_DENOISE_MIN_BATCHES 4

typedef struct rt_denoise_variance_params {
  int32_t passes;      /* as rt_denoise_params.passes */
  int32_t min_batches; /* batches a tile needs before its moments are used; 0: RT_DENOISE_MIN_BATCHES;
                          anything else below 2 counts as 2 */
  double sigma_normal; /* 0: default; < 0: term off */
  double sigma_depth;  /* 0: default; < 0: term off */
  double sigma_hit;    /* 0: default; < 0: term off */
  double sigma_lum;    /* 0: default; < 0: term off; not halved per pass (the variance shrinks instead) */
} rt_denoise_variance_params;

/* Bytes of workspace rt_denoise_variance_device needs for this frame (a
   multiple of 256): four fp32 float4 planes and one float plane, each padded
   to 256 B, 68 B per pixel -- col[0], col[1] = (e.r, e.g, e.b, v), geo, alb
   as rt_denoise_device's, and h. */
int rt_denoise_variance_workspace_bytes(const rt_frame *frame, int64_t *bytes);

/* rt_denoise_device with its colour term replaced.  c, a_d, e, n, h, z and y
   are that function's.  Per pixel a variance v of the luminance of e:
     from moments  when device_s1 and device_s2 are given ([H][W] doubles as
                   rt_adaptive_update_device maintains them, with
                   device_tile_strata and batch_strata >= 1) and the pixel's
                   tile has b = tile_strata[t] / batch_strata >= min_batches
                   batches (integer division):
                   v_c = max(0, (s2 - s1 s1 / b) / (b - 1)) / b and
                   v = v_c / lum(a_d)^2, lum the Rec. 709 luminance.  Dividing
                   the variance of c's luminance by lum(a_d)^2 gives the
                   variance of e's luminance exactly for a grey albedo only;
                   for a coloured albedo it is an approximation.
     spatial       everywhere else: over the 7x7 window at step 1, tap weights
                   exp(-min(x, 80)) with x the normal, depth and hit terms of
                   rt_denoise_device (s = 1, d = max(|di|, |dj|)), the centre
                   1, taps outside the image or with a non-finite e skipped;
                   with d_q = y_q - y_p: m1 = sum w d / sum w,
                   m2 = sum w d^2 / sum w, v = max(0, m2 - m1^2) -- the weighted
                   variance of y over the window (the shift by y_p drops out).
     v = 0 where e is not finite.
   Passes as rt_denoise_device's (B3 taps, step 2^k, the normal, depth and hit
   terms, the NaN rules) with the colour term |y_p - y_q| / (sigma_lum
   sqrt(v~_p) + 1e-6), v~_p the 3x3 Gaussian (1/4, 1/2, 1/4 per axis, step 1)
   of the pass's input v over the in-image pixels whose e is finite,
   renormalised.  The variance is filtered with the colour:
   v'_p = sum w^2 v_q / (sum w)^2, or v_p when sum w = 0.  out = e a_d;
   device_variance_out ([H][W] doubles), unless NULL, takes the final v.
   With sigma_lum < 0 the result is rt_denoise_device's with sigma_color < 0.
   The contracts are rt_denoise_device's: no rt_scene, nothing allocated, no
   state kept, inputs only read, device_out may be device_rgb, the workspace
   256-B aligned.  RT_ERR_INVALID before anything is queued: everything
   rt_denoise_device refuses; exactly one of device_s1 / device_s2 NULL;
   moments without device_tile_strata or with batch_strata < 1; a
   device_variance_out that overlaps the workspace or device_out; a NaN
   parameter. */
int rt_denoise_variance_device(const rt_frame *frame, const double *device_rgb, double rgb_scale,
                               const int32_t *device_tile_strata, const double *device_guides,
                               int32_t guide_strata, const double *device_s1, const double *device_s2,
                               int32_t batch_strata, const rt_denoise_variance_params *params,
                               void *device_workspace, double *device_out, double *device_variance_out,
                               void *hip_stream);

/* ---- temporal reprojection (functions added under ABI 5: no struct or
   signature above changed) --------------------------------------------------
   Carries the displayed image of the previous camera pose into the new pose
   wherever the same first-hit surface is still visible, and blends it with the
   new pose's samples, so that a camera move does not throw the converged frame
   away (rtx/temporal.py drives this and states it in NumPy; DESIGN.md
   "Temporal reprojection"). */

/* The reprojection's defaults: the best point of the sweep of
   tools/temporal_bench.py (DESIGN.md "Temporal reprojection" records it, and
   what that sweep cannot see: its camera move is small, so it barely prices
   ghosting at disocclusions.  A host whose camera moves further per frame
   should pass the sweep's starting point: max_history 32, sigma_depth 0.02,
   sigma_normal 0.35). */
#define RT_TEMPORAL_MAX_HISTORY 64
#define RT_TEMPORAL_SIGMA_DEPTH 0.5
#define RT_TEMPORAL_SIGMA_NORMAL (-1.0) /* off: the sweep's small camera move never paid for it */
#define RT_TEMPORAL_HIT_MIN 0.75

typedef struct rt_temporal_params {
  int32_t max_history; /* cap of the history's sample count n_h; 0: RT_TEMPORAL_MAX_HISTORY;
                          < 0: RT_ERR_INVALID */
  int32_t reserved;
  double sigma_depth;  /* surface test, relative to the distance from the previous camera;
                          0: default; < 0: test off */
  double sigma_normal; /* normal test |n_p - n'_q| <= sigma_normal; 0: default; < 0: test off */
  double hit_min;      /* least hit fraction h of a pixel that takes or leaves history;
                          0: default; < 0: every pixel */
} rt_temporal_params;

/* Bytes of one history for this frame (a multiple of 256): two fp32 float4
   planes, each padded to 256 B, col = (e.r, e.g, e.b, count) first and
   geo = (n.x, n.y, n.z, z) after it.  A history belongs to the rt_frame it
   was written at. */
int rt_history_bytes(const rt_frame *frame, int64_t *bytes);

/* device_out = the new pose's scaled radiance blended with the previous pose's
   history; device_history_out = the history of this frame.  Per pixel p =
   (i, j), with rt_denoise_device's quantities c = rgb * scale (rgb_scale, or
   with device_tile_strata 1 / max(1, strata of the pixel's 8x8 tile)),
   a_d = max(albedo / g, 0.01), e = c / a_d, n = normal / g, h = hits / g,
   z = depth / max(hits, 1), and the current count n_c = strata_now, or with
   device_tile_strata the tile's strata:
     position    d = pixel00_loc + i pixel_delta_u + j pixel_delta_v - center,
                 P = center + z d / |d|: the pixel-centre ray; with defocus or
                 jitter an approximation of where the samples hit.
     projection  into frame_prev (c', pixel00', du', dv'): v = P - c',
                 N' = du' x dv', num = (pixel00' - c') . N', den = v . N';
                 history is possible only if den num > 0 and h >= hit_min;
                 q = c' + (num / den) v - pixel00', x = q . du' / du' . du',
                 y = q . dv' / dv' . dv', r = |v|.
     taps        the four pixels (floor x + a, floor y + b), a, b in {0, 1},
                 of device_history_prev with their bilinear weights w.  A tap
                 is valid when it lies inside the image, its count' > 0, its
                 e' is finite, |n - n'_q|^2 <= sigma_normal^2, and the surface
                 test passes: for |n|^2 >= 0.25 the distance of the tap's own
                 point P'_q = c' + z'_q d'_q / |d'_q| (its pixel-centre ray)
                 from the plane through P, |n / |n| . (P'_q - P)| <=
                 sigma_depth r; otherwise (a medium: guide normal 0)
                 |z'_q - r| <= sigma_depth r.
     history     Wv = sum of the valid w.  Wv > 0: e_h = sum w e'_q / Wv and
                 n_h = min(sum w count'_q, max_history) (the count sum is not
                 renormalised: a partly valid footprint weighs less);
                 otherwise n_h = 0.
     blend       e_out = (n_h e_h + n_c e) / (n_h + n_c), 0 when both counts
                 are 0; device_out = e_out a_d (what rt_denoise_device then
                 takes as device_rgb with rgb_scale 1 and no tile strata);
                 history_out col = (e_out, n_h + n_c), the count stored as 0
                 when h < hit_min or e_out is not finite (a non-finite current
                 e passes through to device_out); geo = (n, z).
   All of this is fp64; only the history planes are fp32.  frame_prev and
   device_history_prev are both NULL when there is no history: then n_h = 0
   everywhere, device_out = c up to the division and multiplication by a_d,
   and a first history is written.  The call keeps nothing: device_history_prev
   is the history committed at the last camera move, every frame at the current
   pose is computed from it and the current accumulator alone, and on a move
   the host makes the last frame's device_history_out the next
   device_history_prev.
   Asynchronous on hip_stream; needs no rt_scene, allocates nothing; runs on
   the current device.  device_rgb, device_guides and device_history_prev are
   only read; device_out may be device_rgb; device_history_out must not overlap
   device_history_prev, nor device_out either history; histories are 256-B
   aligned.  RT_ERR_INVALID, before anything is queued: a null frame_now,
   device_rgb, device_guides, device_history_out or device_out; an empty frame;
   guide_strata < 1; strata_now < 0 without tile strata; exactly one of
   frame_prev and device_history_prev NULL; a frame_prev of another size; a
   misaligned or overlapping history; max_history < 0; a NaN parameter. */
int rt_temporal_device(const rt_frame *frame_now, const double *device_rgb, double rgb_scale,
                       const int32_t *device_tile_strata, int32_t strata_now,
                       const double *device_guides, int32_t guide_strata,
                       const rt_frame *frame_prev, const void *device_history_prev,
                       const rt_temporal_params *params, void *device_history_out,
                       double *device_out, void *hip_stream);

/* ---- temporal variance (functions added under ABI 5: no struct or signature
   above changed) ------------------------------------------------------------
   The two stages above composed: the variance of the displayed estimate is
   carried across camera moves with its colour, and the variance-guided filter
   runs on the blend with that variance, so a blend that holds 64 strata of
   history is filtered as a 64-strata frame and not as a 1-stratum one
   (rtx/temporal.py NumpyOps.temporal_variance and rtx/denoise.py
   NumpyOps.denoise_given_variance state both in NumPy; DESIGN.md "Temporal
   variance").  v is the variance of the Rec. 709 luminance of e = c / a_d, the
   unit of rt_denoise_variance_device. */

/* Bytes of one variance history for this frame (a multiple of 256): a history
   with a third plane -- col, geo (fp32 float4) at the offsets rt_history_bytes
   gives them, then var (fp32 scalars), each padded to 256 B, 36 B per pixel.
   Its first rt_history_bytes bytes are a plain history. */
int rt_history_variance_bytes(const rt_frame *frame, int64_t *bytes);

/* rt_temporal_device on variance histories.  Position, projection, the four
   taps and their validity, Wv, e_h, n_h, n_c, e_out, device_out, col and geo
   are that function's, bit for bit.  Added, per pixel p:
     current     v_c = device_variance_now[p] ([H][W] doubles), or 0 when that
                 is NaN or negative.
     history     Wv > 0: v_h = sum w max(v'_q, 0) / Wv over the valid taps (the
                 same validity; a NaN v'_q counts as 0, and a tap of weight 0
                 adds nothing, an infinite v'_q included).  Linear on purpose, not
                 sum w^2 v' / Wv^2: after one reprojection neighbouring history
                 pixels share taps and are correlated, crediting the
                 interpolation with a variance reduction would compound over
                 moves, and an overestimate only keeps the filter wider.
                 max_history caps n_h and leaves v_h alone.
     blend       with a = n_h / total, b = n_c / total, total = n_h + n_c:
                 v_out = a^2 v_h + b^2 v_c; a term whose count is 0 is dropped,
                 not multiplied; v_out = 0 when total = 0; without history
                 b = 1 and v_out = v_c exactly.
     outputs     device_variance_out[p] = v_out ([H][W] doubles); history_out
                 var = fp32(v_out), stored as 0 wherever the count is stored
                 as 0.
   The contracts and refusals are rt_temporal_device's with the histories'
   size rt_history_variance_bytes in the alignment and overlap checks, and:
   device_variance_now is only read; a null device_variance_now or
   device_variance_out; a device_variance_out that overlaps either history,
   device_variance_now (every lane reads only its own entry, but in place is
   refused all the same) or device_out. */
int rt_temporal_variance_device(const rt_frame *frame_now, const double *device_rgb, double rgb_scale,
                                const int32_t *device_tile_strata, int32_t strata_now,
                                const double *device_guides, int32_t guide_strata,
                                const rt_frame *frame_prev, const void *device_history_prev,
                                const double *device_variance_now, const rt_temporal_params *params,
                                void *device_history_out, double *device_out, double *device_variance_out,
                                void *hip_stream);

/* rt_denoise_variance_device without its estimation stage: v is
   device_variance[p] ([H][W] doubles, only read; a NaN or negative value is 0)
   and 0 where e is not finite; the passes, the remodulation, the outputs and
   the workspace (rt_denoise_variance_workspace_bytes) are that function's.
   params->min_batches is ignored.  Fed with the plane
   rt_denoise_variance_device writes at passes < 0 it gives that function's
   result bit for bit.  RT_ERR_INVALID before anything is queued: everything
   rt_denoise_variance_device refuses of the arguments both take; a null
   device_variance; a device_variance that overlaps the workspace, device_out
   or device_variance_out. */
int rt_denoise_given_variance_device(const rt_frame *frame, const double *device_rgb, double rgb_scale,
                                     const int32_t *device_tile_strata, const double *device_guides,
                                     int32_t guide_strata, const double *device_variance,
                                     const rt_denoise_variance_params *params, void *device_workspace,
                                     double *device_out, double *device_variance_out, void *hip_stream);

/* ---- tile exchange (multi-GPU tile sharding) ------------------------------ */
/* Tile-layout chunk partials [tile][chunk][64][3] (rt_render_device with
   RT_LAYOUT_TILES and strata_chunks = chunks) -> per-tile sums [tile][64][3],
   each added in chunk order on the device.  parts and device_tiles must not
   overlap (unless chunks == 1). */
int rt_tiles_sum_device(const double *device_parts, int64_t n_tiles, int32_t chunks,
                        double *device_tiles, void *hip_stream);

/* Compact tiles of n_shards tile shards -> frame rows on the device: tile t of
   the row range [params->row_begin, row_end) in row-major tile order (shard
   t % n_shards rendered it as its local tile t / n_shards) is read from
   device_tiles[(t % n_shards) * shard_stride + t / n_shards][64][3] and
   written to device_rgb (index (j-row_begin)*W+i), scaled by
   pixel_samples_scale when params->output is RT_OUT_SCALED, added when
   params->accumulate.  shard_stride (tiles) >= ceil(tiles / n_shards): the
   padded per-shard slot of a gather (RCCL gather into [shard][stride]). */
int rt_tiles_to_frame_device(const double *device_tiles, int32_t n_shards, int64_t shard_stride,
                             const rt_frame *frame, const rt_render_params *params,
                             double *device_rgb, void *hip_stream);

/* ---- multi-device rendering (tile shards) -------------------------------- */
typedef struct rt_multi rt_multi; /* opaque: one rt_scene per shard */

/* One scene per shard, shard k on devices[k % n_devices] (n_shards may exceed
   n_devices: virtual shards share a device; at most RT_MULTI_MAX_SHARDS, since
   each shard holds a device copy of the scene and a host thread).  The scenes
   are compiled and uploaded by one host thread per shard; a failure to start
   one returns RT_ERR_DEVICE (nothing is thrown across the ABI). */
#define RT_MULTI_MAX_SHARDS 256
int rt_multi_create(const rt_scene_desc *desc, const int32_t *devices, int32_t n_devices,
                    int32_t n_shards, rt_multi **multi);
/* ... every shard's scene created with `tuning` (NULL: the default) */
int rt_multi_create_tuned(const rt_scene_desc *desc, const int32_t *devices, int32_t n_devices,
                          int32_t n_shards, const rt_tuning *tuning, rt_multi **multi);

/* rt_render over the shards: shard k renders the 8x8 tiles t = k (mod
   n_shards) of the row range, all launched strata, in (tile, stratum chunk)
   work units, on its own host thread, and adds each of its pixels' chunk
   partials in chunk order on its device; the compact tiles are copied device
   to device (xGMI peer copies) to shard 0's device, reordered into the frame
   there (rt_tiles_to_frame_device's kernel) and copied to host_rgb once.  params->tile_first/tile_stride/
   layout must be 0/0-or-1/RT_LAYOUT_FRAME; params->strata_chunks 0 = the chunk
   split rt_render's frame launch uses on shard 0's device, which makes the
   output bit-identical to rt_render on one device.  Synchronous. */
int rt_multi_render(rt_multi *multi, const rt_frame *frame, const rt_render_params *params,
                    double *host_rgb);

/* Device time (ms) of each shard's last render kernel (HIP events on its
   launch stream); ms must hold n_shards doubles (0 for a shard with no tiles). */
int rt_multi_shard_ms(rt_multi *multi, double *ms);

/* Host time (ms) of the last rt_multi_render's exchange: from the slowest
   shard's render completion to the frame assembled on shard 0's device (the
   peer copies and the reorder; the final D2H copy excluded). */
int rt_multi_gather_ms(rt_multi *multi, double *ms);

int rt_multi_destroy(rt_multi *multi);

/* ---- moving spheres (functions added under ABI 5: no struct or signature
   above changed) ------------------------------------------------------------
   A scene is otherwise immutable after rt_scene_create; these move spheres of
   the world without the host compile, upload and BVH build of a new scene.
   The world tree keeps its topology and has every box refitted bottom-up on
   the device from the moved primitives (csrc/rt_refit.hip; DESIGN.md "Moving
   spheres").  The closest hit does not depend on the tree, so the moved scene
   renders what a scene freshly created at the new positions renders (same
   hits; the usual exact-t ties aside); only the tree's quality degrades with
   the distance moved -- rt_scene_bvh_cost tells.

   object_ids index rt_scene_desc.objects.  A sphere is movable when it is
   among the world's primitive items -- directly, through lists or under any
   rotate_y / translate chain -- and does not bound a constant medium.  A
   move sets the sphere's centre at t = 0 in the item's local frame
   (rt_object_desc.a); a moving sphere keeps its displacement c1 - c0, so its
   second centre moves by the same vector; the radius stays.  An entry of the
   lights list that is the same object follows with it.  Tile dispatch orders
   measured before the move are kept: they change the order of the work, never
   a frame.  What the caller accumulated or displayed before the move
   (progressive sums, adaptive moments, display histories) describes the old
   scene: the caller resets it. */

/* centres: n x 3 doubles.  Validates everything first, and on any error leaves
   the scene untouched: an id out of range, an object that is not a sphere
   among the world's primitive items, an id named twice or a centre that is not
   finite is RT_ERR_INVALID; a sphere that bounds a constant medium is
   RT_ERR_UNSUPPORTED (the medium's box and face constants would have to
   follow).  n = 0 is a no-op.  Synchronous: waits for the scene's pending
   launches, and the move has completed on return. */
int rt_scene_move_spheres(rt_scene *scene, int32_t n, const int32_t *object_ids, const double *centres);

/* The same with device arrays, asynchronously on hip_stream (NULL = the HIP
   null stream): the move joins the scene's launch chain like rt_render_device,
   so it never overlaps a render of the scene on any stream.  The arrays are
   read by kernels on hip_stream and may be rewritten by work queued there
   after the call.  An entry the host variant would refuse is skipped on the
   device (both entries of an id named twice); the others are applied.  The
   scene's first move also allocates its refit state (it waits for the scene's
   own stream then). */
int rt_scene_move_spheres_device(rt_scene *scene, int32_t n, const int32_t *device_object_ids,
                                 const double *device_centres, void *hip_stream);

/* rt_scene_move_spheres on every shard's scene.  Host arrays only. */
int rt_multi_move_spheres(rt_multi *multi, int32_t n, const int32_t *object_ids, const double *centres);

/* ---- rebuilding the world BVH (functions added under ABI 5: no struct or
   signature above changed) ---------------------------------------------------
   A refit keeps the topology chosen at creation, and the tree degrades as the
   spheres drift.  rt_scene_rebuild_bvh builds a new tree over the world items
   where they are now, entirely on the device (csrc/rt_bvh_sah.hip, and
   csrc/rt_collapse.hip for a 4-wide scene; DESIGN.md "Rebuild"), without the
   host compile and the uploads of a new scene: the tree, the scene info, the
   SAH cost and therefore every frame are those of a scene freshly created from
   the moved description with bvh_builder = RT_BVH_DEVICE_SAH and the same
   arity and tuning, bit for bit.  Tile dispatch orders are kept.

   Synchronous, like rt_scene_move_spheres: waits for the scene's pending
   launches, and the new tree is live on return.  *rebuilt (may be NULL) is 1
   when the new tree was taken.  It is 0, with RT_OK and the scene exactly as it
   was (its refitted tree), when the world is flat, when the builder makes the
   world one leaf (the scene's kernel instance is fixed at creation), when the
   new tree is deeper than the traversal stack or rt_tuning.lbvh_max_depth
   allows, or when a 4-wide scene's collapse or the LDS plan does not fit at
   the new depth.  The arity never changes; rt_scene_info.bvh_builder becomes
   RT_BVH_DEVICE_SAH.  The first rebuild allocates the scene's rebuild state
   (staging for the tree and the items, the builder's workspace), kept until
   rt_scene_destroy; a scene created by the host builder also gets a node range
   large enough for any tree over its items, counted in
   rt_scene_info.device_bytes.  RT_ERR_INVALID: a null scene.  A device failure
   is RT_ERR_DEVICE. */
int rt_scene_rebuild_bvh(rt_scene *scene, int32_t *rebuilt);

/* rt_scene_rebuild_bvh on every shard's scene; *rebuilt is 1 only if every
   shard took its new tree. */
int rt_multi_rebuild_bvh(rt_multi *multi, int32_t *rebuilt);

/* ---- live transforms and quads (functions added under ABI 5: no struct or
   signature above changed) ---------------------------------------------------
   The Cornell scenes are made of quads, of boxes placed by
   translate(rotate_y(box)), of constant media bounded by such boxes and of a
   quad lamp; these functions move them the way rt_scene_move_spheres moves
   spheres: the new values go into the device tables, every constant medium's
   world box is recomputed from its boundary, and the world tree is refitted
   (csrc/rt_refit.hip; DESIGN.md "Live transforms and quads").  The edited
   scene renders what a scene freshly created from the edited description
   renders (same hits; the usual exact-t ties aside).  rt_scene_rebuild_bvh
   works from the edited tables.  As after a sphere move, tile dispatch orders
   are kept, and what the caller accumulated or displayed before the edit
   describes the old scene: the caller resets it.

   object_ids index rt_scene_desc.objects.

   A RT_OBJ_TRANSLATE or RT_OBJ_ROTATE_Y object is settable when it stands in
   the transform chain of a world primitive, of a world constant medium, of a
   medium's boundary or of an entry of the lights list.  Every place the object
   stands in follows.  values: n x 3 doubles; a translate gets its offset, a
   rotate_y gets (sin, cos, ignored) -- the stored form of rt_object_desc
   (moving == RT_STORED_FORM); rt_rotate_y_sincos gives the pair of an angle.
   A medium's boundary constants do not depend on the transforms above the
   boundary, so a transform inside or above a medium is settable like any other.

   A RT_OBJ_QUAD object is movable when it is among the world's primitive items
   or an entry of the lights list (under any chain), and does not bound a
   constant medium.  A move sets the corner Q (rt_object_desc.a); the sides u
   and v stay, and with them the normal and the area.  A lamp that is one quad
   object in the world and another in the lights list is two objects: the
   caller moves both. */

/* Validates everything first, and on any error leaves the scene untouched: an
   id out of range, an object that is not a translate or rotate_y, one that
   stands in no chain, an id named twice or a value that is not finite is
   RT_ERR_INVALID (the third value of a rotate_y row is not looked at).  n = 0
   is a no-op.  Synchronous: waits for the scene's pending launches, and the
   edit has completed on return. */
int rt_scene_set_transforms(rt_scene *scene, int32_t n, const int32_t *object_ids, const double *values);

/* The same with device arrays, asynchronously on hip_stream (NULL = the HIP
   null stream), a link of the scene's launch chain like
   rt_scene_move_spheres_device.  An entry the host variant would refuse is
   skipped on the device (both entries of an id named twice); the others are
   applied.  The scene's first edit or move also allocates its refit state. */
int rt_scene_set_transforms_device(rt_scene *scene, int32_t n, const int32_t *device_object_ids,
                                   const double *device_values, void *hip_stream);

/* rt_scene_set_transforms on every shard's scene.  Host arrays only. */
int rt_multi_set_transforms(rt_multi *multi, int32_t n, const int32_t *object_ids, const double *values);

/* corners: n x 3 doubles.  Validates everything first, and on any error leaves
   the scene untouched: an id out of range, an object that is not a quad, a
   quad that is neither a world primitive item nor a light entry, an id named
   twice, a corner that is not finite or whose plane constant dot(n, Q) is not
   finite is RT_ERR_INVALID; a quad that bounds a constant medium is
   RT_ERR_UNSUPPORTED (the medium's face constants would have to follow).
   n = 0 is a no-op.  Synchronous, like rt_scene_set_transforms. */
int rt_scene_move_quads(rt_scene *scene, int32_t n, const int32_t *object_ids, const double *corners);

/* The same with device arrays, asynchronously on hip_stream; entries the host
   variant would refuse are skipped. */
int rt_scene_move_quads_device(rt_scene *scene, int32_t n, const int32_t *device_object_ids,
                               const double *device_corners, void *hip_stream);

/* rt_scene_move_quads on every shard's scene.  Host arrays only. */
int rt_multi_move_quads(rt_multi *multi, int32_t n, const int32_t *object_ids, const double *corners);

/* (sin, cos) of a rotate_y angle given in degrees, exactly as scene creation
   computes them from rt_object_desc.s: the row rt_scene_set_transforms takes.
   Needs no scene and no device.  RT_ERR_INVALID (no message is set): a null
   pointer. */
int rt_rotate_y_sincos(double degrees, double *sin_theta, double *cos_theta);

/* ---- ray queries (functions and two structs added under ABI 5: no struct or
   signature above changed) ---------------------------------------------------
   The edit calls above address objects by object_ids; these calls go the
   other way: which object lies along a ray, in the same vocabulary (csrc/
   rt_query.h, rt_query.hip; DESIGN.md "Ray queries").

   The surface found is the render's closest primitive hit of
   Ray{origin, direction, time} over the world's primitive items, in the
   render's range (0.001, inf) in units of `direction` (Camera.cpp:242), with
   the render's own search (rt_path.h trace_closest) and hit record
   (trace_tail): the same tie rules, the same transform chains, moving spheres
   at `time`.  `direction` need not be a unit vector; t counts in its length.

   Constant media are not reported: a query has no RNG key, so a ray passes
   through fog to the surface behind it (the scene's instance with
   RT_FEAT_MEDIA and RT_FEAT_LIGHTS masked).

   t_max: a hit counts when t <= t_max.  +inf, and every t_max <= 0 (-inf
   included), mean no limit; a NaN t_max makes the ray a miss.  The search is
   the unlimited one and its minimum is compared with t_max afterwards.

   A ray with a zero direction, or with a NaN or infinite origin, direction or
   time component, is a miss, decided before anything is walked.

   The result of a ray does not depend on the rays around it, on its position
   in the array, or on the tree (host-built, device-built, refitted, rebuilt,
   binary or 4-wide): it gives the same bytes in every case. */
typedef struct rt_ray {
  double origin[3];
  double direction[3];
  double time;
  double t_max;
} rt_ray; /* 64 B */

typedef struct rt_ray_hit {
  double t;     /* in units of `direction`; +inf for a miss */
  double p[3];  /* origin + t direction, through the item's transform chain */
  double n[3];  /* unit normal against the ray */
  int32_t object;       /* index into rt_scene_desc.objects of the sphere or quad hit:
                           what rt_scene_move_spheres / rt_scene_move_quads take */
  int32_t chain_object; /* the outermost translate or rotate_y above it (the first
                           entry of its chain): what rt_scene_set_transforms takes,
                           and rt_object_desc.child leads from it down to `object`;
                           -1 when the primitive stands under no transform */
  int32_t material;     /* index into rt_scene_desc.materials */
  int32_t front;        /* 1: the ray met the outside of the surface */
} rt_ray_hit; /* 72 B; a miss: t = +inf, p = n = 0, object = chain_object =
                 material = -1, front = 0 */

/* device_hits[k] = the hit of device_rays[k] for k in [0, n): every record is
   written exactly once with plain stores, nothing else is written.  Both
   arrays are device memory of the scene's device, 8-byte aligned.
   Asynchronous on hip_stream (NULL = the HIP null stream); a link of the
   scene's launch chain like rt_render_guides_device: it sees every edit queued
   before it, and rt_scene_destroy waits for it.  Uses none of the scene's
   scratch and allocates nothing.  n = 0 queues nothing and returns RT_OK.
   RT_ERR_INVALID, before anything is queued: a null scene, n < 0, a null
   array with n > 0, n above 2^36. */
int rt_trace_device(rt_scene *scene, int64_t n, const rt_ray *device_rays, rt_ray_hit *device_hits,
                    void *hip_stream);

/* The same with host arrays: staged through device memory on the scene's own
   stream; the hits are in `hits` on return. */
int rt_trace(rt_scene *scene, int64_t n, const rt_ray *rays, rt_ray_hit *hits);

/* rt_trace on shard 0's scene (the shards hold one description). */
int rt_multi_trace(rt_multi *multi, int64_t n, const rt_ray *rays, rt_ray_hit *hits);

/* The ray through the point (x, y) of the frame's pixel grid, the one
   rt_temporal_device reprojects along: (i, j) is the centre of pixel (i, j),
     origin = center,
     direction = pixel00_loc + x pixel_delta_u + y pixel_delta_v - center
   (added left to right), time = 0, t_max = +inf.  No jitter and no defocus.
   Host only: needs no scene and no device.  RT_ERR_INVALID: a null pointer. */
int rt_pixel_ray(const rt_frame *frame, double x, double y, rt_ray *ray);

/* ---- occlusion queries (four functions added under ABI 5: no struct or
   signature above changed) ---------------------------------------------------
   Line of sight, shadow and ambient-occlusion tests want a verdict, not a
   record: is anything in the way (csrc/rt_occlusion.h, rt_occlusion.hip;
   DESIGN.md "Occlusion queries").

   occluded[k] is 1 exactly where rt_trace's record of the same rt_ray is a
   hit, and 0 where it is a miss -- for every ray, not within a tolerance: the
   same hit tests, transform chains, moving spheres at `time`, the same range
   (0.001, t_max] in units of `direction`, constant media passed through, and
   the same rules for t_max (+inf and every t_max <= 0: no limit; NaN:
   unoccluded) and for bad rays (a zero direction, or a NaN or infinite origin,
   direction or time component: unoccluded, decided from the bits before
   anything is walked).

   What differs is the search.  It is an any-hit walk of its own: the interval
   is (0.001, t_max] from the first node on, so a short segment culls every box
   beyond its end, and a ray stops at the first primitive it accepts, whichever
   that is.  The verdict is still a property of the ray and the tables alone:
   it does not depend on the tree (host-built, device-built, refitted, rebuilt,
   binary, 4-wide or flat), on which blocker was met first, on the rays around
   it or on its position in the array.

   Not offered: transmittance through media, a caller t_min, a bit-mask
   output. */

/* device_occluded[k] = the verdict of device_rays[k] for k in [0, n): one
   byte, 0 or 1, each written exactly once with a plain store; nothing else is
   written.  Both arrays are device memory of the scene's device; the rays are
   8-byte aligned, the bytes need no alignment (a bool buffer does).
   Asynchronous on hip_stream (NULL = the HIP null stream); a link of the
   scene's launch chain like rt_trace_device: it sees every edit queued before
   it, and rt_scene_destroy waits for it.  Uses none of the scene's scratch
   and allocates nothing.  n = 0 queues nothing and returns RT_OK.
   RT_ERR_INVALID, before anything is queued: a null scene, n < 0, a null
   array with n > 0, n above 2^36. */
int rt_occluded_device(rt_scene *scene, int64_t n, const rt_ray *device_rays, uint8_t *device_occluded,
                       void *hip_stream);

/* The same with host arrays: staged through device memory on the scene's own
   stream; the verdicts are in `occluded` on return. */
int rt_occluded(rt_scene *scene, int64_t n, const rt_ray *rays, uint8_t *occluded);

/* rt_occluded on shard 0's scene (the shards hold one description). */
int rt_multi_occluded(rt_multi *multi, int64_t n, const rt_ray *rays, uint8_t *occluded);

/* The ray that asks whether b is visible from a:
     origin = a, direction = b - a (componentwise), time as given, t_max = 0.999.
   The search starts at 0.001 in units of `direction`, which skips the surface
   a stands on; 0.999 skips the surface b stands on by the same amount.  a == b
   gives a zero direction and non-finite inputs go through unchanged: both are
   unoccluded by the rule above.  Host only: needs no scene and no device.
   RT_ERR_INVALID: a null pointer. */
int rt_segment_ray(const double a[3], const double b[3], double time, rt_ray *ray);

/* ---- radiance queries (four functions and one struct added under ABI 5: no
   struct or signature above changed) -----------------------------------------
   rt_trace asks for the closest surface along a ray and rt_occluded for any
   blocker; these calls ask what a path tracer exists to answer: how much
   light arrives along the ray (csrc/rt_radiance.h, rt_radiance.hip; DESIGN.md
   "Radiance queries").  Light probes, lightmap texels, a fisheye, orthographic,
   panoramic or stereo camera, a renderer that brings its own primary rays:
   each makes its rt_ray array and gets this library's light transport.

   Per sample.  Sample s of ray k is the render's own path: it starts as
   Ray{origin, direction, time} with weight 1 at bounce 0 and runs the
   render's integrator (rt_path.h segment) until it ends, with the RNG key
   Key{seed; first_key + k, first_sample + s} where the render has
   Key{seed; pixel, stratum}.  The range (0.001, inf) in units of `direction`,
   the media's free-flight draws, light sampling, the max_depth rule and
   miss -> background are the render's; the sample's value is the path's
   terminal weight.  t_max is not read.  The kernel instance is the one the
   scene's renders run (the feature set of rt_scene_info.features, and the
   Lambertian-only form of a plain flat diffuse-only world), with nodes and
   Perlin tables read from memory.

   Per ray.  rgb[k] = +0.0, or its current value when `accumulate`, plus the
   samples, added in ascending s, each channel separately: a raw sum by the
   RT_OUT_SUM convention, the caller scales.  The result is a property of the
   ray, its key and the scene's tables alone: it does not depend on the rays
   around it, on its position in a launch (first_key + k names it), on the tree
   (host-built, device-built, refitted, rebuilt, binary or 4-wide), or on where
   a sample range is split -- samples [0, 4) in one call give the bytes of
   [0, 2) followed by [2, 4) with accumulate.

   Bad rays.  A ray with a zero direction, or with a NaN or infinite origin,
   direction or time component (rt_trace's test, without its rule for t_max:
   t_max is ignored even if NaN), contributes nothing and draws nothing: its
   rgb is 0, or is left as it was under `accumulate`.

   With rt_camera_rays below, first_key = row_begin * image_width,
   first_sample = stratum and samples = 1 re-create one stratum of rt_render
   with RT_OUT_SUM, bit for bit. */
typedef struct rt_radiance_params {
  uint64_t seed;          /* the render's seed: Key{k0,k1} = (lo, hi) */
  uint32_t first_key;     /* Key.pixel of ray k is first_key + k (mod 2^32) */
  int32_t  first_sample;  /* Key.sample of a ray's s-th sample is first_sample + s */
  int32_t  samples;       /* samples per ray, >= 0 */
  int32_t  max_depth;     /* the frame's max_depth; <= 0: every sample is 0 */
  int32_t  accumulate;    /* 0: rgb[k] = sum; 1: rgb[k] += the samples, in order */
  int32_t  _reserved;     /* 0 */
  rt_vec3  background;    /* what a miss returns (rt_frame.background) */
} rt_radiance_params; /* 56 B */

/* device_rgb[3k .. 3k+2] = the sum of device_rays[k] for k in [0, n): every
   one written exactly once with plain stores, nothing else is written.  Both
   arrays are device memory of the scene's device, 8-byte aligned.
   Asynchronous on hip_stream (NULL = the HIP null stream); a link of the
   scene's launch chain like rt_trace_device: it sees every edit queued before
   it, and rt_scene_destroy waits for it.  Uses none of the scene's scratch
   and allocates nothing.  n = 0, and samples = 0 with accumulate, queue
   nothing and return RT_OK.
   RT_ERR_INVALID, before anything is queued: null params; non-zero
   _reserved; samples < 0, first_sample < 0, or first_sample + samples above
   INT32_MAX; n < 0; n above 2^32 (keys must be distinct within a call); a
   null array with n > 0; a null scene. */
int rt_radiance_device(rt_scene *scene, int64_t n, const rt_ray *device_rays, const rt_radiance_params *params,
                       double *device_rgb, void *hip_stream);

/* The same with host arrays: staged through device memory on the scene's own
   stream (with accumulate, rgb goes up too); the sums are in `rgb` on return. */
int rt_radiance(rt_scene *scene, int64_t n, const rt_ray *rays, const rt_radiance_params *params, double *rgb);

/* rt_radiance on shard 0's scene (the shards hold one description). */
int rt_multi_radiance(rt_multi *multi, int64_t n, const rt_ray *rays, const rt_radiance_params *params,
                      double *rgb);

/* The render's own camera ray for every pixel of rows [row_begin, row_end)
   (0, 0: the whole frame), row-major: rays[(j - row_begin) * image_width + i]
   is the ray rt_render traces for stratum `stratum` of pixel (i, j) under
   `seed` -- its jitter inside the stratum's cell, its defocus origin and its
   ray time, from Key{seed; j * image_width + i, stratum} -- with
   t_max = +inf.  Useful on its own (another integrator on the render's rays)
   and with rt_radiance above.  Host only: needs no scene and no device.
   RT_ERR_INVALID: a null pointer, a frame rt_render would refuse, rows outside
   the frame, stratum outside [0, sqrt_spp^2). */
int rt_camera_rays(const rt_frame *frame, uint64_t seed, int32_t stratum, int32_t row_begin, int32_t row_end,
                   rt_ray *rays);

/* ---- object motion vectors (functions and one struct added under ABI 5: no
   struct or signature above changed) ---------------------------------------
   rt_temporal_device reprojects along the camera only: after an edit
   (rt_scene_move_spheres, rt_scene_set_transforms, rt_scene_move_quads) a
   history of the old scene would be blended onto the moved objects.  A pose is
   a snapshot of what those edits write; rt_motion_device gives, per pixel,
   where the surface under it stood at an earlier pose; the _motion forms of
   the temporal calls reproject along camera and object motion together
   (rtx/temporal.py TemporalDisplay.edited drives all of it; DESIGN.md "Object
   motion vectors").  Constant media carry no motion. */

/* Bytes of one pose of this scene: a multiple of 256, at least 256. */
int rt_scene_pose_bytes(const rt_scene *scene, int64_t *bytes);

/* device_pose = the scene's movable state as it stands at this point of the
   scene's launch chain, after every edit queued before the call: (a, b, c) of
   every transform record, c0 of every sphere record and Q of every quad record,
   three doubles each.  The layout is the library's own: only rt_motion_device
   reads it.  It is indexed by table record, not by world item:
   rt_scene_rebuild_bvh permutes the items and leaves the primitive tables where
   they are, so a pose outlives a rebuild.  A pose belongs to the scene it was
   taken from; the caller owns the buffer, the library keeps nothing.
   Asynchronous on hip_stream and a link of the scene's launch chain, like
   rt_scene_move_spheres_device.  RT_ERR_INVALID, before anything is queued: a
   null scene, a null device_pose or one that is not 256-B aligned. */
int rt_scene_pose_device(rt_scene *scene, void *device_pose, void *hip_stream);

typedef struct rt_motion {
  double d[3];  /* where the surface point under the pixel centre was at the pose, minus where it is */
  double dn[3]; /* its unit normal then, minus now */
  double t;     /* rt_trace's t of the pixel-centre ray; +inf: a miss */
  int32_t object, chain_object; /* rt_ray_hit's; -1, -1 for a miss */
} rt_motion; /* 64 B; a miss: d = dn = 0, t = +inf, object = chain_object = -1 */

/* device_motion[j * image_width + i] = the motion of the surface under pixel
   (i, j) since device_pose_prev was taken.  The ray is rt_pixel_ray(frame, i,
   j); t, object and chain_object are the bytes rt_trace_device writes for it
   (constant media are passed through).  The hit is carried into the winning
   item's local frame (the current transform chain), its offset q from the
   primitive's anchor (c0 of a sphere, Q of a quad) and its local normal are
   placed twice by the same operations -- anchor + q, then the chain innermost
   first -- once with the scene's current tables and once with the pose's values
   of the same records: d and dn are the differences.  An object nothing moved
   therefore has d = dn = +0 exactly.  One lane per pixel, every record written
   once with plain stores; uses none of the scene's scratch and allocates
   nothing.  Asynchronous on hip_stream, a link of the scene's launch chain.
   RT_ERR_INVALID, before anything is queued: a null argument; an empty frame;
   a device_pose_prev that is not 256-B aligned; a device_motion that is not
   8-B aligned. */
int rt_motion_device(rt_scene *scene, const rt_frame *frame, const void *device_pose_prev,
                     rt_motion *device_motion, void *hip_stream);

/* rt_temporal_device with object motion: device_motion is rt_motion_device's
   plane for frame_now and the pose device_history_prev was committed at.  A
   pixel whose guide normal is a surface's (|n|^2 >= 0.25), whose record is a
   hit (object >= 0) and whose d and dn are not all zero substitutes
   P_m = P + d for P in the projection (v, den, x, y, r) and in the plane test,
   n_m = n + dn for n in the normal test, and n_m / |n_m| for n / |n| as the
   plane's normal.  Everything written is unchanged: geo = (n, z) is the
   current pose's; the blend and the counts are rt_temporal_device's.  Every
   other pixel (media included) takes rt_temporal_device's path: an all-zero
   plane gives that function's outputs bit for bit.  A non-finite d gives a NaN
   x, which fails the range test: no history.  device_motion is only read and
   may overlap no output.  Refusals: rt_temporal_device's, and a null or
   overlapping device_motion. */
int rt_temporal_motion_device(const rt_frame *frame_now, const double *device_rgb, double rgb_scale,
                              const int32_t *device_tile_strata, int32_t strata_now,
                              const double *device_guides, int32_t guide_strata,
                              const rt_frame *frame_prev, const void *device_history_prev,
                              const rt_motion *device_motion, const rt_temporal_params *params,
                              void *device_history_out, double *device_out, void *hip_stream);

/* rt_temporal_variance_device with object motion, in the same way. */
int rt_temporal_variance_motion_device(const rt_frame *frame_now, const double *device_rgb, double rgb_scale,
                                       const int32_t *device_tile_strata, int32_t strata_now,
                                       const double *device_guides, int32_t guide_strata,
                                       const rt_frame *frame_prev, const void *device_history_prev,
                                       const rt_motion *device_motion, const double *device_variance_now,
                                       const rt_temporal_params *params, void *device_history_out,
                                       double *device_out, double *device_variance_out, void *hip_stream);

/* ---- guided sampling (one function added under ABI 5: no struct or signature
   above changed) ------------------------------------------------------------
   rt_adaptive_select_device retires a tile by the new pose's own batch
   moments; after a camera move that is min_batches batches for every tile,
   whatever history the display carried over.  This rule retires by the error
   of the displayed estimate instead: the blend and the variance that
   rt_temporal_variance_device writes (rtx/guided.py drives it and states it in
   NumPy, NumpyOps.select; DESIGN.md "Guided sampling"). */

/* The rule's defaults (the threshold has none): floor in demodulated units,
   the unit of e = c / a_d. */
#define RT_GUIDED_FLOOR 1e-2
#define RT_GUIDED_MIN_COUNT 8

/* device_tiles_out = the tiles of device_tiles_in[0 .. n_in) that still need
   samples, in input order; *device_count_out = their number (4 bytes).
   device_history is the variance history rt_temporal_variance_device wrote for
   this frame, of which only the col plane (e.r, e.g, e.b, count; fp32) is
   read; device_variance is that call's device_variance_out ([H][W] doubles).
   Per pixel p inside the image, in fp64:
     y = 0.2126 e.r + 0.7152 e.g + 0.0722 e.b;
     v = device_variance[p], 0 when that is NaN or negative;
     rel = sqrt(v) / (y + floor), +inf when a channel of e is not finite or
           the quotient is NaN;
     count_p = max(col.count, n_c), n_c the strata of the pixel's tile
           (max(device_tile_strata[t], 0)), or strata_now without tile strata:
           the stored count is 0 where the hit fraction is below hit_min, and
           such a pixel still holds its own samples.
   Per listed tile t (entries are clamped into [0, tiles - 1]): e_t = the mean
   of rel and c_t = the minimum of count_p over the tile's pixels inside the
   image.  The tile is dropped when c_t >= min_count and e_t <= threshold (a
   NaN e_t keeps it): a tile with one pixel that found no history has
   c_t = n_c and must earn min_count samples at the new pose.
   device_tile_error[t] = e_t and device_tile_count[t] = c_t for the listed
   tiles where those arrays ([tiles] doubles) are given; either may be NULL.
   The 64-lane sum is a butterfly: e_t agrees with a sequential sum to
   rounding, and the same inputs give the same bits again (no atomics).
   n_in = 0 writes a count of 0 and nothing else.  Asynchronous on hip_stream;
   needs no rt_scene, allocates nothing, keeps no state; runs on the current
   device.  The history, the variance, the strata and the input list are only
   read.  RT_ERR_INVALID, before anything is queued: a null frame,
   device_history, device_variance, device_tiles_out or device_count_out, or a
   null device_tiles_in with n_in > 0; an empty frame; n_in < 0 or above the
   frame's tile count; a history that is not 256-B aligned;
   device_tiles_out == device_tiles_in; a NaN threshold, floor or min_count;
   floor <= 0; strata_now < 0. */
int rt_guided_select_device(const rt_frame *frame, const void *device_history, const double *device_variance,
                            const int32_t *device_tile_strata, int32_t strata_now, double threshold,
                            double floor, double min_count, const int32_t *device_tiles_in, int32_t n_in,
                            int32_t *device_tiles_out, int32_t *device_count_out, double *device_tile_error,
                            double *device_tile_count, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
