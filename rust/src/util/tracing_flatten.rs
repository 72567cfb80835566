// tracing_flatten.rs — pasted into src/util/tracing.rs by `include!("tracing_flatten.rs");` (last line of that file).
// Camera -> mi_camera_desc (tracing.rs:138-155, field for field), Scene as an Intersectable (tracing.rs:326: only ever the
// boundary of a ConvexVolume), and the new body of Scene::render_to_image (tracing.rs:221): flatten -> ONE FFI call -> RgbImage.
// Needs: `pub trait Intersectable: super::mi_rt::FlattenObject` (tracing.rs:42) and the reference's own render_to_image
// renamed to render_to_image_cpu (tracing.rs:221).  UNVERIFIED by a compiler (see mi_rt.rs).

use super::mi_rt::{self, FlattenObject, SceneBuilder};

impl Camera {
    pub fn flatten(&self) -> mi_rt::mi_camera_desc {
        mi_rt::mi_camera_desc {
            eyepoint: self.eyepoint.into(), view_dir: self.view_dir.into(), up: self.up.into(),
            projection_mode: match self.projection_mode {
                CameraProjectionMode::Orthographic => mi_rt::MI_PROJ_ORTHOGRAPHIC,
                CameraProjectionMode::Perspective => mi_rt::MI_PROJ_PERSPECTIVE,
            },
            shading_mode: match self.shading_mode {
                ShadingMode::Phong => mi_rt::MI_SHADE_PHONG,
                ShadingMode::PathTrace => mi_rt::MI_SHADE_PATHTRACE,
            },
            path_depth: self.path_depth, path_samples: self.path_samples,
            screen_width: self.screen_width, screen_height: self.screen_height,
            focal_length: self.focal_length, focus_dist: self.focus_dist, lens_radius: self.lens_radius,
            aa_sample_count: self.aa_sample_count, max_trace_dist: self.max_trace_dist, gamma: self.gamma,
        }
    }
}

// A Scene used as an Intersectable is its closest hit over `objects`, first entry wins ties (tracing.rs:330-344): flattened
// as its entries in order.  At top level that IS Scene.objects; inside a ConvexVolume boundary the entries are diverted
// (SceneBuilder::begin_boundary) and become a run of mi_scene_desc.boundary_objects.
impl FlattenObject for Scene {
    fn flatten(&self, out: &mut SceneBuilder) {
        for o in self.objects.iter() { o.flatten(out); }
    }
}

impl Scene {
    /// Everything `render_to_image` needs from `self`, as PODs.  The builder borrows the meshes' arrays from `self`.
    pub fn flatten_scene(&self) -> SceneBuilder {
        let mut sb = SceneBuilder::default();
        for o in self.objects.iter() { o.flatten(&mut sb); }          // Scene.objects order is preserved
        sb
    }

    /// Scene::render_to_image (tracing.rs:221-263) on one MI355X: same signature, same RgbImage layout (tracing.rs:226,254-256).
    /// Panics where the reference panics (tracing.rs:546 unwraps): a scene the GPU path does not take is reported, not
    /// silently rendered some other way — call `render_to_image_cpu()` (the reference's own loop) for those.
    pub fn render_to_image(&self) -> RgbImage {
        self.render_to_image_seeded(rand::random::<u32>(), 1)
    }

    /// `seed` makes the image reproducible (the reference's thread_rng is not); `n_gpus` > 1 cuts the image into 32x32 tiles
    /// over the GPUs of this node (mi_multi_*: replaces rayon's row split, tracing.rs:228) — the same image for every n_gpus.
    pub fn render_to_image_seeded(&self, seed: u32, n_gpus: i32) -> RgbImage {
        let sb = self.flatten_scene();
        if let Some(why) = &sb.unsupported { panic!("mi_rt: this scene cannot run on the GPU path: {}", why); }
        let cam = self.camera.flatten();
        let mut desc = sb.desc();
        desc.point_light_pos = self.point_light_pos.into();          // Scene fields read by ShadingMode::Phong (tracing.rs:282,288,292)
        desc.ambient = self.ambient.into();
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };    // flags 0, max_state_bytes 0 = automatic
        let mut img = RgbImage::new(self.camera.screen_width, self.camera.screen_height);
        let null_f32 = std::ptr::null_mut::<f32>();
        let null_u32 = std::ptr::null_mut::<u32>();
        let null_stats = std::ptr::null_mut::<mi_rt::mi_stats>();
        unsafe {
            assert_eq!(mi_rt::mi_abi_version(), mi_rt::MI_RT_ABI_VERSION, "libmi_rt.so and mi_rt.rs disagree on the ABI");
            let rc;
            if n_gpus <= 1 {
                let mut ctx = std::ptr::null_mut();
                assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
                let up = mi_rt::mi_scene_upload(ctx, &desc);
                rc = if up != 0 { up } else {
                    mi_rt::mi_render(ctx, &cam, &opts, null_f32, img.as_mut_ptr(), null_u32, null_stats)
                };
                let msg = mi_rt::last_error();                         // before destroy: the message is per thread, not per ctx
                mi_rt::mi_ctx_destroy(ctx);
                assert_eq!(rc, 0, "{}", msg);
            } else {
                let mut m = std::ptr::null_mut();
                assert_eq!(mi_rt::mi_multi_create(n_gpus, std::ptr::null(), &mut m), 0, "{}", mi_rt::last_error());
                let up = mi_rt::mi_multi_scene_upload(m, &desc);
                rc = if up != 0 { up } else {
                    mi_rt::mi_multi_render(m, &cam, &opts, null_f32, img.as_mut_ptr(), null_u32, null_stats)
                };
                let msg = mi_rt::last_error();
                mi_rt::mi_multi_destroy(m);
                assert_eq!(rc, 0, "{}", msg);
            }
        }
        img
    }

    /// `impl Intersectable for Scene` (tracing.rs:326-346) for a batch of rays on the GPU (mi_intersect_rays): per ray the index into
    /// `self.objects` of the closest hit in [t_min, t_max] (-1 = None) and RayHit.distance.  `origins` / `dirs` are [x, y, z] per ray;
    /// directions are used as given.  Ray i draws from the stream (seed, first_key + i, 0), which only a ConvexVolume reads.
    pub fn intersect_rays(&self, origins: &[[f32; 3]], dirs: &[[f32; 3]], t_min: f32, t_max: f32, seed: u32, first_key: u32) -> (Vec<i32>, Vec<f32>) {
        assert_eq!(origins.len(), dirs.len(), "mi_rt: origins and dirs differ in length");
        let n = origins.len();
        let mut object = vec![-1i32; n];
        let mut distance = vec![0.0f32; n];
        let (po, pd) = (origins.as_ptr() as *const f32, dirs.as_ptr() as *const f32);
        let (pobj, pt) = (object.as_mut_ptr(), distance.as_mut_ptr());
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_intersect_rays(ctx, n as u32, po, pd, t_min, t_max, seed, first_key, pobj, pt, std::ptr::null_mut(), std::ptr::null_mut(),
                                     std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        });
        (object, distance)
    }

    /// Is `Scene::intersect_ray(ray_i, t_min, t_max_i)` (tracing.rs:326-346) Some?  The any-hit query on the GPU (mi_occluded_rays): a ray
    /// is done at its first accepted hit.  `ray_t_max`, when given, holds one t_max per ray and replaces `t_max`.  Directions are used as
    /// given: the segment a -> b is origin a, dir b - a, [eps, 1 - eps].  Ray i draws from the stream (seed, first_key + i, 0).
    pub fn occluded_rays(&self, origins: &[[f32; 3]], dirs: &[[f32; 3]], t_min: f32, t_max: f32, ray_t_max: Option<&[f32]>, seed: u32,
                         first_key: u32) -> Vec<bool> {
        assert_eq!(origins.len(), dirs.len(), "mi_rt: origins and dirs differ in length");
        let n = origins.len();
        if let Some(t) = ray_t_max { assert_eq!(t.len(), n, "mi_rt: ray_t_max must hold one value per ray"); }
        let mut occluded = vec![0u8; n];
        let (po, pd) = (origins.as_ptr() as *const f32, dirs.as_ptr() as *const f32);
        let pt = ray_t_max.map_or(std::ptr::null(), |t| t.as_ptr());
        let pout = occluded.as_mut_ptr();
        self.with_gpu_scene(|ctx| unsafe { mi_rt::mi_occluded_rays(ctx, n as u32, po, pd, t_min, t_max, pt, seed, first_key, pout) });
        occluded.into_iter().map(|b| b != 0).collect()
    }

    /// Ambient-occlusion baking with rays made on the GPU (mi_hemisphere_occlusion): for every surface point, how many of `n_samples`
    /// hemisphere rays about its normal are NOT occluded within [t_min, t_max], and the sum of the open directions (the bent normal
    /// before normalisation).  Sample s = first_sample + k of point i takes its direction from Lambertian::scatter's sample_hemisphere
    /// on the stream (seed, first_key + i, 2s) and tests the ray with the stream (seed, first_key + i, 2s + 1); the normal and the
    /// direction are used as given.  `world_radius`: t_max is a world-space radius (MI_HEMI_WORLD_RADIUS), not a multiple of |d|.
    /// A bake split by points (first_key advanced) or by samples (first_sample advanced) gives the counts of one call exactly.
    pub fn hemisphere_occlusion(&self, points: &[[f32; 3]], normals: &[[f32; 3]], first_sample: u32, n_samples: u32, t_min: f32, t_max: f32,
                                world_radius: bool, seed: u32, first_key: u32) -> (Vec<u32>, Vec<[f32; 3]>) {
        assert_eq!(points.len(), normals.len(), "mi_rt: points and normals differ in length");
        let n = points.len();
        let mut open = vec![0u32; n];
        let mut bent = vec![[0.0f32; 3]; n];
        let (pp, pn) = (points.as_ptr() as *const f32, normals.as_ptr() as *const f32);
        let (popen, pbent) = (open.as_mut_ptr(), bent.as_mut_ptr() as *mut f32);
        let flags = if world_radius { mi_rt::MI_HEMI_WORLD_RADIUS } else { 0 };
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_hemisphere_occlusion(ctx, n as u32, pp, pn, first_sample, n_samples, t_min, t_max, flags, seed, first_key, popen, pbent)
        });
        (open, bent)
    }

    /// Scene::shade_ray (tracing.rs:300-324) at level 0 for a batch of rays on the GPU (mi_shade_rays): the radiance per ray; the camera
    /// supplies path_depth, path_samples and max_trace_dist.
    pub fn shade_rays(&self, origins: &[[f32; 3]], dirs: &[[f32; 3]], seed: u32, first_key: u32) -> Vec<[f32; 3]> {
        assert_eq!(origins.len(), dirs.len(), "mi_rt: origins and dirs differ in length");
        let n = origins.len();
        let cam = self.camera.flatten();
        let mut rgb = vec![[0.0f32; 3]; n];
        let (po, pd, pout) = (origins.as_ptr() as *const f32, dirs.as_ptr() as *const f32, rgb.as_mut_ptr() as *mut f32);
        self.with_gpu_scene(|ctx| unsafe { mi_rt::mi_shade_rays(ctx, &cam, n as u32, po, pd, seed, first_key, pout) });
        rgb
    }

    /// Scene::render_to_image (tracing.rs:221-263) with a ray table in place of Camera::generate_rays (mi_render_rays): `origins` and
    /// `dirs` hold `rays_per_pixel` x height x width rays, row-major ([s][y][x]), rays_per_pixel = 1 or camera.aa_sample_count (which
    /// need not be a square here).  Sample s of pixel (x, y) draws from the stream (seed, y * width + x, s); directions are used as
    /// given.  The camera's eyepoint, view_dir, up, projection and lens fields are ignored.
    pub fn render_rays(&self, origins: &[[f32; 3]], dirs: &[[f32; 3]], rays_per_pixel: u32, seed: u32) -> RgbImage {
        let n = rays_per_pixel as usize * self.camera.screen_height as usize * self.camera.screen_width as usize;
        assert_eq!(origins.len(), n, "mi_rt: the origins table must hold rays_per_pixel * height * width rays");
        assert_eq!(dirs.len(), n, "mi_rt: the dirs table must hold rays_per_pixel * height * width rays");
        let cam = self.camera.flatten();
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };
        let mut img = RgbImage::new(self.camera.screen_width, self.camera.screen_height);
        let (po, pd, pimg) = (origins.as_ptr() as *const f32, dirs.as_ptr() as *const f32, img.as_mut_ptr());
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_render_rays(ctx, &cam, &opts, po, pd, rays_per_pixel, std::ptr::null_mut(), pimg, std::ptr::null_mut(), std::ptr::null_mut())
        });
        img
    }

    /// Lightmap baking (mi_render_points): `points` and `normals` hold `rows_per_pixel` x height x width texels, row-major ([row][y][x]),
    /// rows_per_pixel = 1 or camera.aa_sample_count.  Sample s of texel (x, y) leaves its point along sample_hemisphere(normal), drawn on
    /// the GPU from the stream (seed, width * height + y * width + x, s), and its path draws from (seed, y * width + x, s): the image
    /// render_rays gives for those directions.  A zero normal marks an empty texel (black).  Points are used as given.
    pub fn render_points(&self, points: &[[f32; 3]], normals: &[[f32; 3]], rows_per_pixel: u32, seed: u32) -> RgbImage {
        let n = rows_per_pixel as usize * self.camera.screen_height as usize * self.camera.screen_width as usize;
        assert_eq!(points.len(), n, "mi_rt: the points table must hold rows_per_pixel * height * width texels");
        assert_eq!(normals.len(), n, "mi_rt: the normals table must hold rows_per_pixel * height * width texels");
        let cam = self.camera.flatten();
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };
        let mut img = RgbImage::new(self.camera.screen_width, self.camera.screen_height);
        let (pp, pn, pimg) = (points.as_ptr() as *const f32, normals.as_ptr() as *const f32, img.as_mut_ptr());
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_render_points(ctx, &cam, &opts, pp, pn, rows_per_pixel, std::ptr::null_mut(), pimg, std::ptr::null_mut(), std::ptr::null_mut())
        });
        img
    }

    /// The lightmap of `mesh` (mi_bake_lightmap): its uv atlas, width x height texels, is rasterised on the GPU into the point table
    /// render_points would take and gathered with `samples` samples per texel, each from its own jittered position inside the texel
    /// (`jitter`) or all from the centre; `offset` lifts the points off the surface along the normal.  Of `mesh` the four arrays, the two
    /// counts and transform are read.  The camera supplies path_depth, max_trace_dist and gamma.  Only the mesh crosses the bus.
    pub fn bake_lightmap(&self, mesh: &mi_rt::mi_mesh, width: u32, height: u32, samples: u32, jitter: bool, offset: f32, seed: u32) -> RgbImage {
        let mut cam = self.camera.flatten();
        cam.screen_width = width;
        cam.screen_height = height;
        cam.aa_sample_count = samples;
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };
        let flags = if jitter { mi_rt::MI_LM_JITTER } else { 0 };
        let mut img = RgbImage::new(width, height);
        let pimg = img.as_mut_ptr();
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_bake_lightmap(ctx, &cam, &opts, mesh, flags, offset, std::ptr::null_mut(), pimg, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        });
        img
    }

    /// Finish a baked lightmap (mi_lightmap_finish): the edge-aware a-trous filter guided by the atlas's centre table (`points`, `normals`:
    /// mi_lightmap_texels with rows = 1, no jitter), then `dilate` passes of gutter dilation.  `image` is the bake's f32 image; all three hold
    /// height x width texels, row-major.  f32::INFINITY turns sigma_plane, reach or sigma_color off.  Returns the finished image and the valid
    /// mask (1 = covered or filled by the dilation).  Needs no scene: an associated function.
    pub fn finish_lightmap(image: &[[f32; 3]], points: &[[f32; 3]], normals: &[[f32; 3]], width: u32, height: u32, levels: u32,
                           normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32, dilate: u32) -> (Vec<[f32; 3]>, Vec<u8>) {
        let n = width as usize * height as usize;
        assert!(image.len() == n && points.len() == n && normals.len() == n, "mi_rt: image, points and normals must hold height * width texels");
        let mut out = vec![[0.0f32; 3]; n];
        let mut valid = vec![0u8; n];
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_finish(ctx, width, height, image.as_ptr() as *const f32, points.as_ptr() as *const f32,
                                               normals.as_ptr() as *const f32, levels, normal_power_log2, sigma_plane, reach, sigma_color, dilate,
                                               out.as_mut_ptr() as *mut f32, valid.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, valid)
    }

    /// bake_lightmap with the second moments (mi_bake_lightmap_moments): returns the bake's f32 mean and, per texel and channel, the mean of
    /// the squares of its `samples` samples, both height x width texels, row-major: what finish_lightmap_var takes.
    pub fn bake_lightmap_moments(&self, mesh: &mi_rt::mi_mesh, width: u32, height: u32, samples: u32, jitter: bool, offset: f32,
                                 seed: u32) -> (Vec<[f32; 3]>, Vec<[f32; 3]>) {
        let mut cam = self.camera.flatten();
        cam.screen_width = width;
        cam.screen_height = height;
        cam.aa_sample_count = samples;
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };
        let flags = if jitter { mi_rt::MI_LM_JITTER } else { 0 };
        let n = width as usize * height as usize;
        let mut mean = vec![[0.0f32; 3]; n];
        let mut m2 = vec![[0.0f32; 3]; n];
        let (pmean, pm2) = (mean.as_mut_ptr() as *mut f32, m2.as_mut_ptr() as *mut f32);
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_bake_lightmap_moments(ctx, &cam, &opts, mesh, flags, offset, pm2, pmean, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        });
        (mean, m2)
    }

    /// Finish a baked lightmap with the variance-guided colour weight (mi_lightmap_finish_var): finish_lightmap whose colour weight is
    /// `sigma_color` standard errors of each texel's own mean wide (plus `color_floor`; f32::INFINITY turns the weight off), from the bake's
    /// second moments `m2` and sample count `samples`.  Returns the finished image, its per-texel variance and the valid mask.
    pub fn finish_lightmap_var(image: &[[f32; 3]], m2: &[[f32; 3]], samples: u32, points: &[[f32; 3]], normals: &[[f32; 3]], width: u32,
                               height: u32, levels: u32, normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32,
                               color_floor: f32, dilate: u32) -> (Vec<[f32; 3]>, Vec<f32>, Vec<u8>) {
        let n = width as usize * height as usize;
        assert!(image.len() == n && m2.len() == n && points.len() == n && normals.len() == n,
                "mi_rt: image, m2, points and normals must hold height * width texels");
        let mut out = vec![[0.0f32; 3]; n];
        let mut var = vec![0.0f32; n];
        let mut valid = vec![0u8; n];
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_finish_var(ctx, width, height, image.as_ptr() as *const f32, m2.as_ptr() as *const f32, samples,
                                                   points.as_ptr() as *const f32, normals.as_ptr() as *const f32, levels, normal_power_log2,
                                                   sigma_plane, reach, sigma_color, color_floor, dilate, out.as_mut_ptr() as *mut f32,
                                                   var.as_mut_ptr(), valid.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, var, valid)
    }

    /// The adaptive bake (mi_bake_lightmap_adaptive): every texel gets `first_samples` samples, then up to `max_rounds` rounds of
    /// `round_samples` more go to the texels whose blurred standard error exceeds `target_rel` times their luminance plus `target_abs`.
    /// Returns the merged mean, the merged means of squares and the samples behind each texel: what finish_lightmap_var_counts takes.
    pub fn bake_lightmap_adaptive(&self, mesh: &mi_rt::mi_mesh, width: u32, height: u32, first_samples: u32, round_samples: u32, max_rounds: u32,
                                  target_rel: f32, target_abs: f32, jitter: bool, offset: f32, seed: u32) -> (Vec<[f32; 3]>, Vec<[f32; 3]>, Vec<u32>) {
        let mut cam = self.camera.flatten();
        cam.screen_width = width;
        cam.screen_height = height;
        cam.aa_sample_count = first_samples;
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };
        let ad = mi_rt::mi_lightmap_adaptive { first_samples: first_samples, round_samples: round_samples, max_rounds: max_rounds,
                                               target_rel: target_rel, target_abs: target_abs };
        let flags = if jitter { mi_rt::MI_LM_JITTER } else { 0 };
        let n = width as usize * height as usize;
        let mut mean = vec![[0.0f32; 3]; n];
        let mut m2 = vec![[0.0f32; 3]; n];
        let mut counts = vec![0u32; n];
        let (pmean, pm2, pcounts) = (mean.as_mut_ptr() as *mut f32, m2.as_mut_ptr() as *mut f32, counts.as_mut_ptr());
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_bake_lightmap_adaptive(ctx, &cam, &opts, mesh, flags, offset, &ad, pcounts, pm2, pmean, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        });
        (mean, m2, counts)
    }

    /// finish_lightmap_var for an adaptive bake (mi_lightmap_finish_var_counts): `counts` holds every texel's own sample count in the
    /// place of `samples`.  Returns the finished image, its per-texel variance and the valid mask.
    pub fn finish_lightmap_var_counts(image: &[[f32; 3]], m2: &[[f32; 3]], counts: &[u32], points: &[[f32; 3]], normals: &[[f32; 3]], width: u32,
                                      height: u32, levels: u32, normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32,
                                      color_floor: f32, dilate: u32) -> (Vec<[f32; 3]>, Vec<f32>, Vec<u8>) {
        let n = width as usize * height as usize;
        assert!(image.len() == n && m2.len() == n && counts.len() == n && points.len() == n && normals.len() == n,
                "mi_rt: image, m2, counts, points and normals must hold height * width texels");
        let mut out = vec![[0.0f32; 3]; n];
        let mut var = vec![0.0f32; n];
        let mut valid = vec![0u8; n];
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_finish_var_counts(ctx, width, height, image.as_ptr() as *const f32, m2.as_ptr() as *const f32,
                                                          counts.as_ptr(), points.as_ptr() as *const f32, normals.as_ptr() as *const f32,
                                                          levels, normal_power_log2, sigma_plane, reach, sigma_color, color_floor, dilate,
                                                          out.as_mut_ptr() as *mut f32, var.as_mut_ptr(), valid.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, var, valid)
    }

    /// Light probes (mi_render_probes): `points` holds `rows_per_pixel` x height x width probe positions, row-major ([row][y][x]),
    /// rows_per_pixel = 1 or camera.aa_sample_count.  Sample s of probe (x, y) leaves its point along rand_sphere_vec (what
    /// Isotropic::scatter returns: uniform over the sphere), drawn on the GPU from the stream (seed, width * height + y * width + x, s),
    /// and its path draws from (seed, y * width + x, s).  Returns the SH L2 radiance coefficients, height x width records of
    /// [coefficient 0..9][channel r, g, b], in the basis order of mi_rt.h.
    pub fn render_probes(&self, points: &[[f32; 3]], rows_per_pixel: u32, seed: u32) -> Vec<[[f32; 3]; 9]> {
        let n = self.camera.screen_height as usize * self.camera.screen_width as usize;
        assert_eq!(points.len(), rows_per_pixel as usize * n, "mi_rt: the points table must hold rows_per_pixel * height * width probes");
        let cam = self.camera.flatten();
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };
        let mut sh = vec![[[0.0f32; 3]; 9]; n];
        let (pp, psh) = (points.as_ptr() as *const f32, sh.as_mut_ptr() as *mut f32);
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_render_probes(ctx, &cam, &opts, pp, rows_per_pixel, psh, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        });
        sh
    }

    /// Sample an irradiance volume (mi_probe_volume_sample): `sh` holds the first nx * ny * nz records of render_probes' result for
    /// the probe grid of the box [lo, hi] (probe (i, j, k) has number (k * ny + j) * nx + i and sits at the centre of its cell), `valid`
    /// is empty (every probe takes part) or one byte per probe (0 = takes no part).  Every point is lit through its normal: trilinear
    /// interpolation of the eight probes around it, convolved with the clamped cosine lobe; `normal_weight` sets MI_PV_NORMAL_WEIGHT.
    /// An all-zero normal marks an empty texel (+0.0, weight 0).  Returns the irradiance and the weight sum per point (0: every corner
    /// was invalid).  Needs no scene: an associated function.
    pub fn sample_probe_volume(lo: [f32; 3], hi: [f32; 3], counts: [u32; 3], sh: &[[[f32; 3]; 9]], valid: &[u8], normal_weight: bool,
                               points: &[[f32; 3]], normals: &[[f32; 3]]) -> (Vec<[f32; 3]>, Vec<f32>) {
        let n = counts[0] as usize * counts[1] as usize * counts[2] as usize;
        assert!(sh.len() == n && (valid.is_empty() || valid.len() == n), "mi_rt: sh (and valid) must hold nx * ny * nz probes");
        assert_eq!(points.len(), normals.len(), "mi_rt: one normal per point");
        let volume = mi_rt::mi_probe_volume {
            lo: lo, hi: hi, counts: counts, flags: if normal_weight { mi_rt::MI_PV_NORMAL_WEIGHT } else { 0 },
            sh: sh.as_ptr() as *const f32, valid: if valid.is_empty() { std::ptr::null() } else { valid.as_ptr() },
        };
        let mut out = vec![[0.0f32; 3]; points.len()];
        let mut weight = vec![0.0f32; points.len()];
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_probe_volume_sample(ctx, &volume, points.len() as u32, points.as_ptr() as *const f32,
                                                   normals.as_ptr() as *const f32, out.as_mut_ptr() as *mut f32, weight.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, weight)
    }

    /// A directional lightmap (mi_bake_lightmap_sh): bake_lightmap that returns, per texel, the SH L2 radiance records (render_probes'
    /// basis and order, scaled for the hemisphere's uniform directions) and the f32 mean, both height x width texels, row-major.
    /// eval_lightmap_sh turns the records into the irradiance at any normal.
    pub fn bake_lightmap_sh(&self, mesh: &mi_rt::mi_mesh, width: u32, height: u32, samples: u32, jitter: bool, offset: f32,
                            seed: u32) -> (Vec<[[f32; 3]; 9]>, Vec<[f32; 3]>) {
        let mut cam = self.camera.flatten();
        cam.screen_width = width;
        cam.screen_height = height;
        cam.aa_sample_count = samples;
        let opts = mi_rt::mi_render_opts { seed: seed, rank: 0, world: 1, ..Default::default() };
        let flags = if jitter { mi_rt::MI_LM_JITTER } else { 0 };
        let n = width as usize * height as usize;
        let mut sh = vec![[[0.0f32; 3]; 9]; n];
        let mut mean = vec![[0.0f32; 3]; n];
        let (psh, pmean) = (sh.as_mut_ptr() as *mut f32, mean.as_mut_ptr() as *mut f32);
        self.with_gpu_scene(|ctx| unsafe {
            mi_rt::mi_bake_lightmap_sh(ctx, &cam, &opts, mesh, flags, offset, psh, pmean, std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut(), std::ptr::null_mut())
        });
        (sh, mean)
    }

    /// Finish a directional lightmap (mi_lightmap_finish_sh): finish_lightmap for SH L2 records; the colour weight is taken from the three
    /// k = 0 coefficients and one weight per tap serves all 27 channels.  Returns the finished records and the valid mask.  Needs no
    /// scene: an associated function.
    pub fn finish_lightmap_sh(sh: &[[[f32; 3]; 9]], points: &[[f32; 3]], normals: &[[f32; 3]], width: u32, height: u32, levels: u32,
                              normal_power_log2: u32, sigma_plane: f32, reach: f32, sigma_color: f32, dilate: u32) -> (Vec<[[f32; 3]; 9]>, Vec<u8>) {
        let n = width as usize * height as usize;
        assert!(sh.len() == n && points.len() == n && normals.len() == n, "mi_rt: sh, points and normals must hold height * width texels");
        let mut out = vec![[[0.0f32; 3]; 9]; n];
        let mut valid = vec![0u8; n];
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_finish_sh(ctx, width, height, sh.as_ptr() as *const f32, points.as_ptr() as *const f32,
                                                  normals.as_ptr() as *const f32, levels, normal_power_log2, sigma_plane, reach, sigma_color, dilate,
                                                  out.as_mut_ptr() as *mut f32, valid.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, valid)
    }

    /// The irradiance of a directional lightmap (mi_lightmap_sh_eval): one SH L2 record and one normal per point (an atlas with its own
    /// normal table gives the plain irradiance map, normal-mapped normals the detail).  An all-zero normal gives +0.0; the result is not
    /// clamped.  Needs no scene: an associated function.
    pub fn eval_lightmap_sh(sh: &[[[f32; 3]; 9]], normals: &[[f32; 3]]) -> Vec<[f32; 3]> {
        assert_eq!(sh.len(), normals.len(), "mi_rt: one normal per record");
        let mut out = vec![[0.0f32; 3]; normals.len()];
        if normals.is_empty() { return out; }
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_sh_eval(ctx, normals.len() as u32, sh.as_ptr() as *const f32, normals.as_ptr() as *const f32,
                                                out.as_mut_ptr() as *mut f32);
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        out
    }

    /// Read a finished lightmap at uv points (mi_lightmap_sample): `image` holds height * width texels of `channels` floats (3 or 27), `uv`
    /// intersect's tex_coords as they stand (row 0 is v = 1), `valid` is empty (every texel takes part) or finish_lightmap's mask.
    /// Bilinear over the valid texels, or with `nearest` (MI_LS_NEAREST) the texel Texture::sample addresses.  Returns `channels` floats
    /// per point and the weight sum per point (0: nothing to read).  Needs no scene: an associated function.
    pub fn sample_lightmap(image: &[f32], valid: &[u8], width: u32, height: u32, channels: u32, uv: &[[f32; 2]], nearest: bool) -> (Vec<f32>, Vec<f32>) {
        let texels = width as usize * height as usize;
        assert!(image.len() == texels * channels as usize && (valid.is_empty() || valid.len() == texels), "mi_rt: image (and valid) must hold height * width texels");
        let mut out = vec![0.0f32; uv.len() * channels as usize];
        let mut weight = vec![0.0f32; uv.len()];
        if uv.is_empty() { return (out, weight); }
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_sample(ctx, width, height, channels, image.as_ptr(), if valid.is_empty() { std::ptr::null() } else { valid.as_ptr() },
                                               uv.len() as u32, uv.as_ptr() as *const f32, if nearest { mi_rt::MI_LS_NEAREST } else { 0 },
                                               out.as_mut_ptr(), weight.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, weight)
    }

    /// The irradiance of a finished directional lightmap at uv points and their normals (mi_lightmap_sh_sample): sample_lightmap and
    /// eval_lightmap_sh in one pass; a hit's shading normal shows its normal map.  An all-zero normal gives +0.0 and weight 0.  Returns
    /// the irradiance and the weight sum per point.  Needs no scene: an associated function.
    pub fn sample_lightmap_sh(sh: &[[[f32; 3]; 9]], valid: &[u8], width: u32, height: u32, uv: &[[f32; 2]], normals: &[[f32; 3]],
                              nearest: bool) -> (Vec<[f32; 3]>, Vec<f32>) {
        let texels = width as usize * height as usize;
        assert!(sh.len() == texels && (valid.is_empty() || valid.len() == texels), "mi_rt: sh (and valid) must hold height * width texels");
        assert_eq!(uv.len(), normals.len(), "mi_rt: one normal per point");
        let mut out = vec![[0.0f32; 3]; uv.len()];
        let mut weight = vec![0.0f32; uv.len()];
        if uv.is_empty() { return (out, weight); }
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_sh_sample(ctx, width, height, sh.as_ptr() as *const f32, if valid.is_empty() { std::ptr::null() } else { valid.as_ptr() },
                                                  uv.len() as u32, uv.as_ptr() as *const f32, normals.as_ptr() as *const f32,
                                                  if nearest { mi_rt::MI_LS_NEAREST } else { 0 }, out.as_mut_ptr() as *mut f32, weight.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, weight)
    }

    /// The mip chain's layout (include/mi_rt.h "lightmap mips"): (width, height, offset in texels) of levels 0 .. levels - 1, ceil halving,
    /// levels 1 .. tightly one after the other (level 0 is the image itself: offset 0); `levels` 0 is the full chain.
    pub fn lightmap_mip_layout(width: u32, height: u32, levels: u32) -> Vec<(u32, u32, usize)> {
        let full = 1 + (32 - (width.max(height) - 1).leading_zeros());
        assert!(width >= 1 && height >= 1 && width <= 32768 && height <= 32768 && levels <= full, "mi_rt: size or levels out of range");
        let mut out = Vec::new();
        let mut off = 0usize;
        for l in 0..(if levels == 0 { full } else { levels }) {
            let (w, h) = ((width + (1 << l) - 1) >> l, (height + (1 << l) - 1) >> l);
            out.push((w, h, off));
            if l > 0 { off += w as usize * h as usize; }
        }
        out
    }

    /// The coverage-aware mip chain of a finished lightmap (mi_lightmap_mips): `image` holds height * width texels of `channels` floats
    /// (3 or 27), `valid` is empty (every texel takes part) or finish_lightmap's mask, `levels` counts level 0 (0: the full chain).
    /// Returns levels 1 .. tightly packed as lightmap_mip_layout lays them out: (mips, mip_valid, mip_coverage).  Needs no scene.
    pub fn lightmap_mips(image: &[f32], valid: &[u8], width: u32, height: u32, channels: u32, levels: u32) -> (Vec<f32>, Vec<u8>, Vec<f32>) {
        let texels = width as usize * height as usize;
        assert!(image.len() == texels * channels as usize && (valid.is_empty() || valid.len() == texels), "mi_rt: image (and valid) must hold height * width texels");
        let made: usize = Self::lightmap_mip_layout(width, height, levels).iter().skip(1).map(|l| l.0 as usize * l.1 as usize).sum();
        let mut mips = vec![0.0f32; made.max(1) * channels as usize];
        let mut mip_valid = vec![0u8; made.max(1)];
        let mut coverage = vec![0.0f32; made.max(1)];
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_mips(ctx, width, height, channels, image.as_ptr(), if valid.is_empty() { std::ptr::null() } else { valid.as_ptr() },
                                             levels, mips.as_mut_ptr(), mip_valid.as_mut_ptr(), coverage.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        mips.truncate(made * channels as usize); mip_valid.truncate(made); coverage.truncate(made);
        (mips, mip_valid, coverage)
    }

    /// Read a lightmap's mip chain at uv points and levels of detail (mi_lightmap_sample_lod): sample_lightmap's arguments with the chain
    /// lightmap_mips returned (`mips`, `mip_valid`: empty = every texel valid) and one `lod` per point; trilinear over the valid texels.
    /// Returns `channels` floats per point and the weight sum per point.  Needs no scene.
    pub fn sample_lightmap_lod(image: &[f32], valid: &[u8], width: u32, height: u32, channels: u32, levels: u32, mips: &[f32], mip_valid: &[u8],
                               uv: &[[f32; 2]], lod: &[f32]) -> (Vec<f32>, Vec<f32>) {
        let texels = width as usize * height as usize;
        assert!(image.len() == texels * channels as usize && (valid.is_empty() || valid.len() == texels), "mi_rt: image (and valid) must hold height * width texels");
        let made: usize = Self::lightmap_mip_layout(width, height, levels).iter().skip(1).map(|l| l.0 as usize * l.1 as usize).sum();
        assert!(mips.len() == made * channels as usize && (mip_valid.is_empty() || mip_valid.len() == made), "mi_rt: mips (and mip_valid) must hold levels 1 .. of the layout");
        assert_eq!(uv.len(), lod.len(), "mi_rt: one lod per point");
        let mut out = vec![0.0f32; uv.len() * channels as usize];
        let mut weight = vec![0.0f32; uv.len()];
        if uv.is_empty() { return (out, weight); }
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_sample_lod(ctx, width, height, channels, image.as_ptr(), if valid.is_empty() { std::ptr::null() } else { valid.as_ptr() },
                                                   levels, if mips.is_empty() { std::ptr::null() } else { mips.as_ptr() },
                                                   if mip_valid.is_empty() { std::ptr::null() } else { mip_valid.as_ptr() }, uv.len() as u32,
                                                   uv.as_ptr() as *const f32, lod.as_ptr(), 0, out.as_mut_ptr(), weight.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, weight)
    }

    /// The irradiance of a directional lightmap's mip chain at uv points, their normals and levels of detail (mi_lightmap_sh_sample_lod):
    /// sample_lightmap_sh's arguments with the chain lightmap_mips returned at 27 channels and one `lod` per point.  Needs no scene.
    pub fn sample_lightmap_sh_lod(sh: &[[[f32; 3]; 9]], valid: &[u8], width: u32, height: u32, levels: u32, mips: &[f32], mip_valid: &[u8],
                                  uv: &[[f32; 2]], normals: &[[f32; 3]], lod: &[f32]) -> (Vec<[f32; 3]>, Vec<f32>) {
        let texels = width as usize * height as usize;
        assert!(sh.len() == texels && (valid.is_empty() || valid.len() == texels), "mi_rt: sh (and valid) must hold height * width texels");
        let made: usize = Self::lightmap_mip_layout(width, height, levels).iter().skip(1).map(|l| l.0 as usize * l.1 as usize).sum();
        assert!(mips.len() == made * 27 && (mip_valid.is_empty() || mip_valid.len() == made), "mi_rt: mips (and mip_valid) must hold levels 1 .. of the layout");
        assert!(uv.len() == normals.len() && uv.len() == lod.len(), "mi_rt: one normal and one lod per point");
        let mut out = vec![[0.0f32; 3]; uv.len()];
        let mut weight = vec![0.0f32; uv.len()];
        if uv.is_empty() { return (out, weight); }
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_sh_sample_lod(ctx, width, height, sh.as_ptr() as *const f32, if valid.is_empty() { std::ptr::null() } else { valid.as_ptr() },
                                                      levels, if mips.is_empty() { std::ptr::null() } else { mips.as_ptr() },
                                                      if mip_valid.is_empty() { std::ptr::null() } else { mip_valid.as_ptr() }, uv.len() as u32,
                                                      uv.as_ptr() as *const f32, normals.as_ptr() as *const f32, lod.as_ptr(), 0,
                                                      out.as_mut_ptr() as *mut f32, weight.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, weight)
    }

    /// Packed lightmaps (include/mi_rt.h "packed lightmaps").  `pack_lightmap` and `unpack_lightmap` are the formats' definitions on the
    /// host, in integer and f32 arithmetic alone (a storage conversion needs no device); the bytes equal mi_lightmap_pack's and
    /// mi_lightmap_unpack's bit for bit.  `texels` is [n][channels] f32, channels 3 or 27 (MI_LP_RGB9E5: 3); the result is n * channels
    /// u16 for MI_LP_F16, n u32 for MI_LP_RGB9E5, as the little-endian bytes the C calls take.
    pub fn pack_lightmap(texels: &[f32], format: u32, channels: u32) -> Vec<u8> {
        Self::check_packed_format(format, channels);
        assert!(texels.len() % channels as usize == 0, "mi_rt: texels must be [n][channels]");
        let pow2 = |e: i32| f32::from_bits(((e + 127) as u32) << 23);
        let mut out = Vec::with_capacity(texels.len() * 2);
        if format == mi_rt::MI_LP_F16 {
            for &x in texels { out.extend_from_slice(&Self::f16_bits(x).to_le_bytes()); }
            return out;
        }
        for t in texels.chunks_exact(3) {
            let mut c = [0.0f32; 3];
            for k in 0..3 { c[k] = if t[k] != t[k] { 0.0 } else { t[k].max(0.0).min(65408.0) }; }
            let m = c[0].max(c[1]).max(c[2]);
            let eb = ((m.to_bits() >> 23) & 255) as i32 - 127;
            let ep = eb.max(-16) + 16;
            let ms = (m * pow2(24 - ep) + 0.5).floor();
            let e = ep + (ms == 512.0) as i32;
            let s = pow2(24 - e);
            let mut w = (e as u32) << 27;
            for k in 0..3 { w |= ((c[k] * s + 0.5).floor() as u32) << (9 * k); }
            out.extend_from_slice(&w.to_le_bytes());
        }
        out
    }

    /// The exact decode of `pack_lightmap`'s bytes: [n][channels] f32.
    pub fn unpack_lightmap(packed: &[u8], format: u32, channels: u32) -> Vec<f32> {
        Self::check_packed_format(format, channels);
        let pow2 = |e: i32| f32::from_bits(((e + 127) as u32) << 23);
        if format == mi_rt::MI_LP_F16 {
            assert!(packed.len() % (2 * channels as usize) == 0, "mi_rt: packed must hold whole texels");
            return packed.chunks_exact(2).map(|b| {
                let h = u16::from_le_bytes([b[0], b[1]]) as u32;
                let (sign, ex, man) = ((h & 0x8000) << 16, (h >> 10) & 31, h & 1023);
                if ex == 31 { f32::from_bits(sign | 0x7F80_0000 | if man != 0 { 0x0040_0000 | man << 13 } else { 0 }) }
                else if ex != 0 { f32::from_bits(sign | (ex + 112) << 23 | man << 13) }
                else { f32::from_bits(sign | (man as f32 * pow2(-24)).to_bits()) }
            }).collect();
        }
        assert!(packed.len() % 4 == 0, "mi_rt: packed must hold whole texels");
        let mut out = Vec::with_capacity(packed.len() / 4 * 3);
        for b in packed.chunks_exact(4) {
            let w = u32::from_le_bytes([b[0], b[1], b[2], b[3]]);
            let s = pow2((w >> 27) as i32 - 24);
            for k in 0..3 { out.push(((w >> (9 * k)) & 511) as f32 * s); }
        }
        out
    }

    /// Read a packed lightmap at uv points through mi_lightmap_sample_packed: `sample_lightmap_lod`'s arguments with `image` and `mips` as
    /// `pack_lightmap` made them; an empty `lod` reads level 0 alone (then `levels` must be 1 and `mips` empty, and `nearest` is allowed).
    /// Equals `sample_lightmap(_lod)` on the unpacked texels bit for bit.
    pub fn sample_lightmap_packed(format: u32, image: &[u8], valid: &[u8], width: u32, height: u32, channels: u32, levels: u32, mips: &[u8],
                                  mip_valid: &[u8], uv: &[[f32; 2]], lod: &[f32], nearest: bool) -> (Vec<f32>, Vec<f32>) {
        Self::packed_lookup(format, image, valid, width, height, channels, levels, mips, mip_valid, uv, None, lod, nearest)
    }

    /// The irradiance of a directional lightmap packed as MI_LP_F16 through mi_lightmap_sh_sample_packed: `sample_lightmap_sh_lod`'s
    /// arguments with packed records; an empty `lod` reads level 0 alone.
    pub fn sample_lightmap_sh_packed(format: u32, sh: &[u8], valid: &[u8], width: u32, height: u32, levels: u32, mips: &[u8], mip_valid: &[u8],
                                     uv: &[[f32; 2]], normals: &[[f32; 3]], lod: &[f32], nearest: bool) -> (Vec<[f32; 3]>, Vec<f32>) {
        assert!(uv.len() == normals.len(), "mi_rt: one normal per point");
        let (flat, weight) = Self::packed_lookup(format, sh, valid, width, height, 0, levels, mips, mip_valid, uv, Some(normals), lod, nearest);
        (flat.chunks_exact(3).map(|e| [e[0], e[1], e[2]]).collect(), weight)
    }

    fn check_packed_format(format: u32, channels: u32) {
        assert!(format == mi_rt::MI_LP_F16 || format == mi_rt::MI_LP_RGB9E5, "mi_rt: format must be MI_LP_F16 or MI_LP_RGB9E5");
        assert!(channels == 3 || channels == 27, "mi_rt: channels must be 3 or 27");
        assert!(format != mi_rt::MI_LP_RGB9E5 || channels == 3, "mi_rt: MI_LP_RGB9E5 holds 3 unsigned channels");
    }

    /// f32 -> binary16 bits as the header defines them: a NaN is 0x7E00, everything else is clamped to +-65504 and rounded to nearest even.
    fn f16_bits(x: f32) -> u16 {
        if x != x { return 0x7E00; }
        let u = x.max(-65504.0).min(65504.0).to_bits();
        let (sign, mag) = ((u >> 16) & 0x8000, u & 0x7FFF_FFFF);
        if mag >= 0x3880_0000 {
            let r = mag + 0x0FFF + ((mag >> 13) & 1);
            return (sign | ((r >> 13) - (112 << 10))) as u16;
        }
        if mag < 0x3300_0000 { return sign as u16; }
        let (man, shift) = ((mag & 0x007F_FFFF) | 0x0080_0000, 126 - (mag >> 23));
        let (q, rest, half) = (man >> shift, man & ((1 << shift) - 1), 1 << (shift - 1));
        (sign | (q + (rest > half || (rest == half && q & 1 == 1)) as u32)) as u16
    }

    fn packed_lookup(format: u32, image: &[u8], valid: &[u8], width: u32, height: u32, channels: u32, levels: u32, mips: &[u8], mip_valid: &[u8],
                     uv: &[[f32; 2]], normals: Option<&[[f32; 3]]>, lod: &[f32], nearest: bool) -> (Vec<f32>, Vec<f32>) {
        let (in_c, out_c) = if channels == 0 { (27, 3) } else { (channels, channels) };
        Self::check_packed_format(format, in_c);
        let bytes = if format == mi_rt::MI_LP_F16 { 2 * in_c as usize } else { 4 };
        let texels = width as usize * height as usize;
        assert!(image.len() == texels * bytes && (valid.is_empty() || valid.len() == texels), "mi_rt: image (and valid) must hold height * width texels");
        let made: usize = Self::lightmap_mip_layout(width, height, levels).iter().skip(1).map(|l| l.0 as usize * l.1 as usize).sum();
        assert!(mips.len() == made * bytes && (mip_valid.is_empty() || mip_valid.len() == made), "mi_rt: mips (and mip_valid) must hold levels 1 .. of the layout");
        assert!(lod.is_empty() || lod.len() == uv.len(), "mi_rt: lod is empty or holds one value per point");
        let mut out = vec![0.0f32; uv.len() * out_c as usize];
        let mut weight = vec![0.0f32; uv.len()];
        if uv.is_empty() { return (out, weight); }
        let or_null = |s: &[u8]| if s.is_empty() { std::ptr::null() } else { s.as_ptr() };
        let d = if lod.is_empty() { std::ptr::null() } else { lod.as_ptr() };
        let flags = if nearest { mi_rt::MI_LS_NEAREST } else { 0 };
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = match normals {
                Some(n) => mi_rt::mi_lightmap_sh_sample_packed(ctx, format, width, height, image.as_ptr() as *const std::ffi::c_void, or_null(valid), levels,
                                                               or_null(mips) as *const std::ffi::c_void, or_null(mip_valid), uv.len() as u32,
                                                               uv.as_ptr() as *const f32, n.as_ptr() as *const f32, d, flags, out.as_mut_ptr(),
                                                               weight.as_mut_ptr()),
                None => mi_rt::mi_lightmap_sample_packed(ctx, format, width, height, channels, image.as_ptr() as *const std::ffi::c_void, or_null(valid), levels,
                                                         or_null(mips) as *const std::ffi::c_void, or_null(mip_valid), uv.len() as u32,
                                                         uv.as_ptr() as *const f32, d, flags, out.as_mut_ptr(), weight.as_mut_ptr()),
            };
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, weight)
    }

    /// BC6H lightmaps (include/mi_rt.h "BC6H lightmaps").  `encode_lightmap_bc6h` and `decode_lightmap_bc6h` are the format's definitions on
    /// the host, one level per call, in integer arithmetic alone after the binary16 conversion; the bytes equal mi_lightmap_bc6h_encode's
    /// and mi_lightmap_bc6h_decode's.  `image` is [height][width][3] f32, `valid` empty (every texel takes part) or [height][width],
    /// `rounds` 0 .. 4; the result is ceil(height / 4) x ceil(width / 4) blocks of 16 bytes, row-major.
    pub fn encode_lightmap_bc6h(image: &[f32], valid: &[u8], width: u32, height: u32, rounds: u32) -> Vec<u8> {
        let (w, h) = (width as usize, height as usize);
        assert!(width >= 1 && width <= 32768 && height >= 1 && height <= 32768 && image.len() == w * h * 3 && (valid.is_empty() || valid.len() == w * h),
                "mi_rt: image must be [height][width][3] with 1 .. 32768 texels a side, valid empty or [height][width]");
        assert!(rounds <= mi_rt::MI_BC6H_MAX_ROUNDS, "mi_rt: rounds must be in 0 .. 4");
        let (bw, bh) = ((w + 3) >> 2, (h + 3) >> 2);
        let mut out = Vec::with_capacity(bw * bh * 16);
        for by in 0..bh {
            for bx in 0..bw {
                let mut hb = [[0i64; 3]; 16];
                let mut part = [false; 16];
                for t in 0..16 {
                    let (x, y) = (4 * bx + (t & 3), 4 * by + (t >> 2));
                    if x >= w || y >= h { continue; }
                    let q = y * w + x;
                    if !valid.is_empty() && valid[q] == 0 { continue; }
                    part[t] = true;
                    for k in 0..3 {
                        let v = image[3 * q + k];
                        hb[t][k] = Self::f16_bits(if v > 0.0 { v.min(65504.0) } else { 0.0 }) as i64;
                    }
                }
                out.extend_from_slice(&Self::bc6h_encode_block(&hb, &part, rounds));
            }
        }
        out
    }

    /// The exact decode of a level's blocks: [height][width][3] f32; a block whose low five bits are not 3 gives zeros.
    pub fn decode_lightmap_bc6h(blocks: &[u8], width: u32, height: u32) -> Vec<f32> {
        let (w, h) = (width as usize, height as usize);
        let (bw, bh) = ((w + 3) >> 2, (h + 3) >> 2);
        assert!(width >= 1 && width <= 32768 && height >= 1 && height <= 32768 && blocks.len() == bw * bh * 16,
                "mi_rt: blocks must be ceil(height / 4) x ceil(width / 4) x 16 bytes");
        let pow2 = |e: i32| f32::from_bits(((e + 127) as u32) << 23);
        let mut out = vec![0.0f32; w * h * 3];
        for y in 0..h {
            for x in 0..w {
                let at = ((y >> 2) * bw + (x >> 2)) * 16;
                let v = u128::from_le_bytes(blocks[at..at + 16].try_into().unwrap());
                let t = (y & 3) * 4 + (x & 3);
                let i = (if t == 0 { (v >> 65) & 7 } else { (v >> (64 + 4 * t)) & 15 }) as usize;
                for k in 0..3 {
                    let a = Self::bc6h_unq(((v >> (5 + 10 * k)) & 1023) as i64);
                    let b = Self::bc6h_unq(((v >> (35 + 10 * k)) & 1023) as i64);
                    let hb = if v & 31 == 3 { Self::bc6h_interp(a, b, Self::BC6H_W[i]) as u32 } else { 0 };
                    out[3 * (y * w + x) + k] = if hb >> 10 != 0 { f32::from_bits(((hb >> 10) + 112) << 23 | (hb & 1023) << 13) } else { hb as f32 * pow2(-24) };
                }
            }
        }
        out
    }

    /// The one rule for block counts and offsets of a BC6H chain: (blocks per row, block rows, offset in blocks) of every level of
    /// `lightmap_mip_layout`; level 0 is a buffer of its own (offset 0), levels 1 .. lie one after the other in a second one.
    pub fn lightmap_bc6h_layout(width: u32, height: u32, levels: u32) -> Vec<(u32, u32, usize)> {
        let mut off = 0usize;
        Self::lightmap_mip_layout(width, height, levels).iter().enumerate().map(|(l, m)| {
            let (bw, bh) = ((m.0 + 3) >> 2, (m.1 + 3) >> 2);
            let at = off;
            if l > 0 { off += bw as usize * bh as usize; }
            (bw, bh, if l > 0 { at } else { 0 })
        }).collect()
    }

    /// Read a BC6H lightmap at uv points through mi_lightmap_sample_bc6h: `sample_lightmap_packed`'s arguments, three channels, the levels
    /// as `encode_lightmap_bc6h` made them (level 0 in `image`, levels 1 .. one after the other in `mips`); an empty `lod` reads level 0
    /// alone.  Equals `sample_lightmap(_lod)` on the decoded texels bit for bit.
    pub fn sample_lightmap_bc6h(image: &[u8], valid: &[u8], width: u32, height: u32, levels: u32, mips: &[u8], mip_valid: &[u8],
                                uv: &[[f32; 2]], lod: &[f32], nearest: bool) -> (Vec<[f32; 3]>, Vec<f32>) {
        let layout = Self::lightmap_bc6h_layout(width, height, levels);
        let texels = width as usize * height as usize;
        let made: usize = Self::lightmap_mip_layout(width, height, levels).iter().skip(1).map(|l| l.0 as usize * l.1 as usize).sum();
        let made_blocks: usize = layout.iter().skip(1).map(|l| l.0 as usize * l.1 as usize).sum();
        assert!(image.len() == layout[0].0 as usize * layout[0].1 as usize * 16 && (valid.is_empty() || valid.len() == texels), "mi_rt: image (and valid) must hold level 0");
        assert!(mips.len() == made_blocks * 16 && (mip_valid.is_empty() || mip_valid.len() == made), "mi_rt: mips (and mip_valid) must hold levels 1 .. of the layout");
        assert!(lod.is_empty() || lod.len() == uv.len(), "mi_rt: lod is empty or holds one value per point");
        let mut out = vec![[0.0f32; 3]; uv.len()];
        let mut weight = vec![0.0f32; uv.len()];
        if uv.is_empty() { return (out, weight); }
        let or_null = |s: &[u8]| if s.is_empty() { std::ptr::null() } else { s.as_ptr() };
        let d = if lod.is_empty() { std::ptr::null() } else { lod.as_ptr() };
        let flags = if nearest { mi_rt::MI_LS_NEAREST } else { 0 };
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let rc = mi_rt::mi_lightmap_sample_bc6h(ctx, width, height, image.as_ptr() as *const std::ffi::c_void, or_null(valid), levels,
                                                    or_null(mips) as *const std::ffi::c_void, or_null(mip_valid), uv.len() as u32,
                                                    uv.as_ptr() as *const f32, d, flags, out.as_mut_ptr() as *mut f32, weight.as_mut_ptr());
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
        (out, weight)
    }

    const BC6H_W: [i64; 16] = [0, 4, 9, 13, 17, 21, 26, 30, 34, 38, 43, 47, 51, 55, 60, 64];
    fn bc6h_unq(q: i64) -> i64 { if q == 0 { 0 } else if q == 1023 { 0xFFFF } else { ((q << 16) + 0x8000) >> 10 } }
    fn bc6h_interp(a: i64, b: i64, w: i64) -> i64 { (((a * (64 - w) + b * w + 32) >> 6) * 31) >> 6 }
    fn bc6h_to_c(h: i64) -> i64 { (64 * h + 30) / 31 }

    /// The field whose unquantised value is nearest to c (clamped to 0 .. 65535), the lower field on a tie.
    fn bc6h_quant(c: i64) -> i64 {
        let c = c.max(0).min(65535);
        let q0 = ((c - 1) >> 6).max(0).min(1023);
        let mut best = (q0 - 1).max(0);
        let mut bd = (Self::bc6h_unq(best) - c).abs();
        for step in 0..2 {
            let q = (q0 + step).min(1023);
            let d = (Self::bc6h_unq(q) - c).abs();
            if d < bd { best = q; bd = d; }
        }
        best
    }

    /// Every texel's index for the fields f: the least squared distance to its target, the lowest index on a tie; returns the indices
    /// and the error summed over the texels that take part.
    fn bc6h_assign(target: &[[i64; 3]; 16], part: &[bool; 16], f: &[[i64; 3]; 2]) -> ([usize; 16], i64) {
        let mut idx = [0usize; 16];
        let mut err = 0i64;
        for t in 0..16 {
            let mut be = -1i64;
            for i in 0..16 {
                let mut e = 0i64;
                for k in 0..3 {
                    let d = target[t][k] - Self::bc6h_interp(Self::bc6h_unq(f[0][k]), Self::bc6h_unq(f[1][k]), Self::BC6H_W[i]);
                    e += d * d;
                }
                if be < 0 || e < be { be = e; idx[t] = i; }
            }
            if part[t] { err += be; }
        }
        (idx, err)
    }

    fn bc6h_encode_block(h: &[[i64; 3]; 16], part: &[bool; 16], rounds: u32) -> [u8; 16] {
        let n = part.iter().filter(|&&p| p).count() as i64;
        if n == 0 { return 3u128.to_le_bytes(); }
        let mut sum = [0i64; 3];
        for t in 0..16 { if part[t] { for k in 0..3 { sum[k] += h[t][k]; } } }
        let (mut fi, mut fj, mut far) = (0usize, 0usize, -1i64);
        for i in 0..16 {
            for j in i..16 {
                if !part[i] || !part[j] { continue; }
                let d: i64 = (0..3).map(|k| (h[i][k] - h[j][k]) * (h[i][k] - h[j][k])).sum();
                if d > far { far = d; fi = i; fj = j; }
            }
        }
        let mut f = [[0i64; 3]; 2];
        let mut target = [[0i64; 3]; 16];
        let mut ct = [[0i64; 3]; 16];
        for k in 0..3 {
            f[0][k] = Self::bc6h_quant(Self::bc6h_to_c(h[fi][k]));
            f[1][k] = Self::bc6h_quant(Self::bc6h_to_c(h[fj][k]));
            for t in 0..16 {
                target[t][k] = if part[t] { h[t][k] } else { sum[k] / n };
                ct[t][k] = Self::bc6h_to_c(h[t][k]);
            }
        }
        if f[0] == f[1] {
            for k in 0..3 {                                  // a flat start: the two fields around c where the one is far from it
                let c = Self::bc6h_to_c(h[fi][k]);
                if (Self::bc6h_unq(f[0][k]) - c).abs() > 32 { f[0][k] = if c < 96 { 0 } else { 1022 }; f[1][k] = f[0][k] + 1; }
            }
        }
        let (mut idx, mut err) = Self::bc6h_assign(&target, part, &f);
        for _ in 0..rounds {
            let (mut suu, mut suv, mut svv) = (0i64, 0i64, 0i64);
            let (mut suc, mut svc) = ([0i64; 3], [0i64; 3]);
            for t in 0..16 {
                if !part[t] { continue; }
                let v = Self::BC6H_W[idx[t]];
                let u = 64 - v;
                suu += u * u; suv += u * v; svv += v * v;
                for k in 0..3 { suc[k] += u * ct[t][k]; svc[k] += v * ct[t][k]; }
            }
            let det = suu * svv - suv * suv;
            let mut cf = f;
            if det != 0 {
                for k in 0..3 {
                    cf[0][k] = Self::bc6h_quant((2 * (64 * (svv * suc[k] - suv * svc[k])) + det).div_euclid(2 * det));
                    cf[1][k] = Self::bc6h_quant((2 * (64 * (suu * svc[k] - suv * suc[k])) + det).div_euclid(2 * det));
                }
            }
            let (cidx, cerr) = Self::bc6h_assign(&target, part, &cf);
            if cerr < err { f = cf; idx = cidx; err = cerr; }
        }
        if idx[0] >= 8 {
            f.swap(0, 1);
            for t in 0..16 { idx[t] = 15 - idx[t]; }
        }
        let mut v = 3u128;
        for k in 0..6 { v |= (f[k / 3][k % 3] as u128) << (5 + 10 * k); }
        v |= (idx[0] as u128) << 65;
        for t in 1..16 { v |= (idx[t] as u128) << (64 + 4 * t); }
        v.to_le_bytes()
    }

    /// flatten -> context on device 0 -> upload -> `call` -> destroy; panics with the library's message on failure.
    fn with_gpu_scene<F: FnOnce(*mut mi_rt::mi_ctx) -> i32>(&self, call: F) {
        let sb = self.flatten_scene();
        if let Some(why) = &sb.unsupported { panic!("mi_rt: this scene cannot run on the GPU path: {}", why); }
        let mut desc = sb.desc();
        desc.point_light_pos = self.point_light_pos.into();
        desc.ambient = self.ambient.into();
        unsafe {
            let mut ctx = std::ptr::null_mut();
            assert_eq!(mi_rt::mi_ctx_create(0, &mut ctx), 0, "{}", mi_rt::last_error());
            let up = mi_rt::mi_scene_upload(ctx, &desc);
            let rc = if up != 0 { up } else { call(ctx) };
            let msg = mi_rt::last_error();
            mi_rt::mi_ctx_destroy(ctx);
            assert_eq!(rc, 0, "{}", msg);
        }
    }
}
