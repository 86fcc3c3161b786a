"""The reference's `ImaginationEngine` (dream2real.py:43-358) on the MI355X library, all three calls a user makes:
`build_scene_model` (frames, scene-bound masks, label masks, the label census, camera poses, physics models, captions),
`interpret_user_instr` (movable and relevant objects, lazy physics models, the two visual models, the task masks) and
`dream_best_pose` (physics pre-filter, renderer, `optimise_pose_grid`, the three text files), in the reference's order and
with its switches.  `PathConfig.from_json` reads the reference's settings files.

The models the reference downloads enter from outside: segmentation as a `proposer` (SAM's mask generator alone) and a
`tracker` (XMem alone) with the first label image built between them on the GPU, or as a `segmentor(rgbs, depths)` callable, or
the XMem_masks cache, captioning as a `captions` list or the captions.json cache, the LLM as a `lang_model` object (any
object with `parse_instr`, `get_movable_obj_idx`, `get_relevant_obj_idxs`; `CachedLangModel` answers from a JSON file), CLIP
as `scorer` (+ text embeddings, or a text encoder and tokenizer).  NeRF training still raises: camera poses come from
opt_cam_poses.npy or, with `use_vis_pcds`, from poses.txt, and NeRF visual models from their snapshot cache.  The
cost-volume and best-pose pictures that follow the path (:360-400) are an option of `dream_best_pose` (`vis_cost_vol`); robot
execution stays outside.  `ctx` (an
engine.Context) stands where the reference talks to PyBullet, Open3D and pyngp.
"""
from __future__ import annotations

import dataclasses
import json
import os
from typing import Optional, Sequence

import numpy as np

from . import clip_scoring, combined_rendering, physics_utils


@dataclasses.dataclass
class PathConfig:
    """The `cfg` fields the engine reads (reference dream2real.py:40-99, cfg.py)."""
    data_dir: str
    sample_res: Sequence[int]
    scene_type: int = 0
    render_cam_pose_idx: Sequence[int] = (0,)
    use_phys: bool = True
    lazy_phys_mods: bool = True
    embodied: bool = False
    use_cache_renders: bool = False
    use_cache_goal_pose: bool = False
    spatial_smoothing: bool = True
    physics_only: bool = False
    use_vis_pcds: bool = False
    resolution: Optional[Sequence[int]] = None         # renderer resolution (w, h); None = the reference's 336 x 336
    save_renders: bool = True                          # cb_render/cb_rgb_%04d.png per valid pose (the reference always does: clip_scoring.py:140)
    # what build_scene_model and interpret_user_instr read (cfg.py:19-53, 75-81)
    render_distractors: bool = False
    pcds_type: Optional[int] = None                    # 0: the view single_view_idx alone, 1: every view; None without use_vis_pcds
    single_view_idx: int = 0
    use_cache_dynamic_masks: bool = False
    use_cache_segs: bool = False
    use_cache_cam_poses: bool = False
    use_cache_captions: bool = False
    use_cache_phys: bool = False
    use_cache_vis: bool = False
    use_cache_llm: bool = False
    use_phys_tsdf: bool = True
    multi_view_captions: bool = False
    scene_centre: Optional[Sequence[float]] = None
    scene_phys_bounds: Optional[Sequence[Sequence[float]]] = None      # [[xmin, ymin, zmin], [xmax, ymax, zmax]]
    width: int = 1280
    height: int = 720
    phys_backend: str = "hulls"                        # physics_utils.PHYS_BACKENDS; not a key of the reference's files
    # VIS_BACKENDS; not a key of the reference's files.  An init-only variable stored as a plain attribute: dataclasses.fields() and
    # asdict() keep listing the settings format's fields and phys_backend, as tests/test_engine_host.py pins them
    vis_backend: dataclasses.InitVar[str] = "default"
    # CAM_POSE_REFINES; not a key of the reference's files, held as vis_backend is
    cam_pose_refine: dataclasses.InitVar[str] = "none"

    VIS_BACKENDS = ("default", "tsdf")                 # default: NeRF snapshots, or the clouds of use_vis_pcds; tsdf: colour volumes, ray-cast
    CAM_POSE_REFINES = ("none", "tsdf")                # none: the loader's poses as they are; tsdf: refined against the volume fused so far

    def __post_init__(self, vis_backend, cam_pose_refine):
        if vis_backend not in self.VIS_BACKENDS:
            raise ValueError(f"vis_backend {vis_backend!r} is not one of {self.VIS_BACKENDS}")
        if vis_backend == "tsdf" and self.use_vis_pcds:
            raise ValueError('vis_backend "tsdf" and use_vis_pcds are two different visual models: set one of them')
        if cam_pose_refine not in self.CAM_POSE_REFINES:
            raise ValueError(f"cam_pose_refine {cam_pose_refine!r} is not one of {self.CAM_POSE_REFINES}")
        if cam_pose_refine == "tsdf" and self.use_cache_cam_poses:
            raise ValueError('cam_pose_refine "tsdf" and use_cache_cam_poses conflict: the cached opt_cam_poses.npy would be read and '
                             "nothing refined; set one of them")
        if cam_pose_refine == "tsdf" and not (self.use_vis_pcds or vis_backend == "tsdf"):
            raise ValueError('cam_pose_refine "tsdf" refines the loader\'s poses, which the engine takes only with use_vis_pcds or '
                             'vis_backend "tsdf"; the NeRF backend expects the poses its training optimised')
        self.vis_backend = vis_backend
        self.cam_pose_refine = cam_pose_refine

    # engine keys read as they are; pcds_type, single_view_idx and phys_backend have their own rules below
    _ENGINE_KEYS = ("sample_res", "scene_type", "render_cam_pose_idx", "use_phys", "lazy_phys_mods", "use_cache_renders",
                    "use_cache_goal_pose", "spatial_smoothing", "physics_only", "use_vis_pcds", "render_distractors",
                    "use_cache_dynamic_masks", "use_cache_segs", "use_cache_cam_poses", "use_cache_captions", "use_cache_phys",
                    "use_cache_vis", "use_cache_llm", "use_phys_tsdf", "multi_view_captions", "scene_centre", "scene_phys_bounds")

    @classmethod
    def from_json(cls, config_file, data_dir, **overrides):
        """The reference's settings format (configs/*/*.json) as cfg.py:19-53, 75-81 reads it: the `engine` group and the
        frame size of the `camera` group; `trainer`, `vis`, `robot` and the rest are not read.  `single_view_idx` defaults
        to 0, `pcds_type` is read only with `use_vis_pcds`, `engine.phys_backend`, `engine.vis_backend` and `engine.cam_pose_refine` are this package's own optional keys.  A key
        the path needs and the file lacks is a KeyError naming group.key.  `overrides` set the fields no file carries
        (embodied, resolution, save_renders) or replace what was read."""
        with open(config_file) as f:
            config = json.load(f)

        def need(group, key):
            if group not in config or key not in config[group]:
                raise KeyError(f"{group}.{key}")
            return config[group][key]

        fields = {key: need("engine", key) for key in cls._ENGINE_KEYS}
        fields["pcds_type"] = need("engine", "pcds_type") if fields["use_vis_pcds"] else None
        fields["single_view_idx"] = config["engine"].get("single_view_idx", 0)
        fields["phys_backend"] = config["engine"].get("phys_backend", "hulls")
        fields["vis_backend"] = config["engine"].get("vis_backend", "default")
        fields["cam_pose_refine"] = config["engine"].get("cam_pose_refine", "none")
        fields["width"], fields["height"] = need("camera", "w"), need("camera", "h")
        fields.update(overrides)
        return cls(data_dir=data_dir, **fields)


class CachedLangModel:
    """A language model that answers from a JSON file of {method: {key: answer}}: the three calls interpret_user_instr
    makes, each keyed by the JSON text of its argument list (`key`).  `record` adds an answer, `save` writes the file; a
    question the file does not hold is a KeyError naming the method and the key."""

    METHODS = ("parse_instr", "get_movable_obj_idx", "get_relevant_obj_idxs")

    def __init__(self, path):
        self.path = path
        self.answers = {m: {} for m in self.METHODS}
        if os.path.exists(path):
            with open(path) as f:
                for method, table in json.load(f).items():
                    if method not in self.METHODS:
                        raise ValueError(f"{path}: unknown method {method!r} (expected one of {self.METHODS})")
                    self.answers[method].update(table)

    @staticmethod
    def key(*args) -> str:
        return json.dumps(list(args), ensure_ascii=False, separators=(",", ":"))

    def record(self, method, args, answer):
        if method not in self.METHODS:
            raise ValueError(f"unknown method {method!r} (expected one of {self.METHODS})")
        self.answers[method][self.key(*args)] = answer
        return self

    def save(self):
        with open(self.path, "w") as f:
            json.dump(self.answers, f, indent=1, ensure_ascii=False)

    def _answer(self, method, *args):
        k = self.key(*args)
        if k not in self.answers[method]:
            raise KeyError(f"{self.path}: no cached answer for {method}{k}")
        return self.answers[method][k]

    def parse_instr(self, user_instr):
        """-> (goal_caption, norm_caption)"""
        goal_caption, norm_caption = self._answer("parse_instr", user_instr)
        return goal_caption, norm_caption

    def get_movable_obj_idx(self, user_instr, obj_captions):
        return int(self._answer("get_movable_obj_idx", user_instr, list(obj_captions)))

    def get_relevant_obj_idxs(self, norm_caption, obj_captions, movable_obj_idx):
        return [int(i) for i in self._answer("get_relevant_obj_idxs", norm_caption, list(obj_captions), int(movable_obj_idx))]


def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def compose_checks(checks):
    """reference dream2real.py:296-302: a list of validity checks -> one check that ANDs them in order"""
    def composed_check(pose_batch, task_model, valid_so_far):
        valid_so_far = valid_so_far.clone()
        for check in checks:
            valid_so_far &= check(pose_batch, task_model, valid_so_far)
        return valid_so_far
    return composed_check


class ImaginationEngine:
    """The reference's ImaginationEngine: build_scene_model, interpret_user_instr, dream_best_pose."""

    def __init__(self, cfg: PathConfig, ctx, scorer, *, text_embeds=None, text_encoder=None, tokenizer=None, depths_gt=None,
                 lang_model=None, segmentor=None, intrinsics=None, captioner=None, proposer=None, tracker=None):
        self.cfg, self.ctx, self.scorer = cfg, ctx, scorer
        self.text_embeds, self.text_encoder, self.tokenizer = text_embeds, text_encoder, tokenizer
        self.depths_gt = depths_gt                       # [L, h, w] sensor depth of the render views (dream2real.py:117-118), or None
        self.data_dir = cfg.data_dir
        self.lang_model, self.segmentor = lang_model, segmentor
        # captioner: callable(list of uint8 [h,w,3] thumbnails) -> list of captions, or None, or "clip": a caption.ClipCaptioner built
        # from the engine's own scorer, text encoder and tokenizer names the objects from a closed vocabulary
        if isinstance(captioner, str):
            if captioner != "clip":
                raise ValueError(f"ImaginationEngine: captioner= is a callable or \"clip\", got {captioner!r}")
            missing = [n for n, v in (("scorer", scorer), ("text_encoder=", text_encoder), ("tokenizer=", tokenizer)) if v is None]
            if missing:
                raise ValueError("ImaginationEngine: captioner=\"clip\" names the objects with the CLIP towers, " + " and ".join(missing) +
                                 (" is" if len(missing) == 1 else " are") + " missing")
            from . import caption
            captioner = caption.ClipCaptioner(ctx, scorer, text_encoder, tokenizer)
        self.captioner = captioner
        if (proposer is None) != (tracker is None):
            raise ValueError("ImaginationEngine: proposer= and tracker= come together, " +
                             ("tracker=" if tracker is None else "proposer=") + " is missing")
        # proposer: callable(uint8 [W,H,3], frame 0 turned upright) -> bool [M,W,H] mask proposals (SAM's mask generator alone), or
        # "geometric": what stands above the support plane in frame 0's depth, on the GPU (segmentation.propose_masks, DESIGN.md
        # section 2l; table-top scenes only);
        # tracker: callable(rgbs, labels0 uint8 [H,W]) -> uint8 [N,H,W] raw label images (XMem alone), or "geometric": the labels
        # are carried through the scan by depth and pose on the GPU (segmentation.track_labels)
        if isinstance(tracker, str) and tracker != "geometric":
            raise ValueError(f"ImaginationEngine: tracker= is a callable or \"geometric\", got {tracker!r}")
        if isinstance(proposer, str):
            if proposer != "geometric":
                raise ValueError(f"ImaginationEngine: proposer= is a callable or \"geometric\", got {proposer!r}")
            if cfg.scene_type not in (0, 3):
                raise ValueError(f"ImaginationEngine: proposer=\"geometric\" takes what stands above one support plane for the objects, "
                                 f"which holds for the table-top scenes (scene_type 0 and 3); scene_type {cfg.scene_type} (the shelf: "
                                 f"several boards) has no single plane, pass a callable proposer")
        self.proposer, self.tracker = proposer, tracker
        if intrinsics is None:
            from .scene import INTRINSICS_REALSENSE_1280
            intrinsics = INTRINSICS_REALSENSE_1280
        self.intrinsics = np.asarray(intrinsics, np.float64)
        self.topdown = cfg.scene_type in (0, 3)                                                  # :69
        self.scene_model = None
        self.out_scene_bound_masks = None
        self.static_phys_handles = None
        self.movable_phys_handle = None
        self.renderer = None

    def build_scene_model(self, raw_data=None, *, captions=None):
        """reference dream2real.py:101-177.  raw_data: (rgbs uint8 [N,H,W,3], depths [N,H,W] metres, T_WC [N,4,4]), default the
        frames of data_dir.  captions: one name per object, "__background__" first; default: with captioner= the engine's captioner
        on the GPU-built thumbnails (caption.caption_objs; captions.json is written, or read under use_cache_captions), else the
        captions.json of data_dir.
        Sets self.scene_model, self.out_scene_bound_masks and self.depths_gt."""
        import torch
        from . import segmentation
        from .data_loader import d2r_dataloader
        from .scene_model import ObjectModel, SceneModel
        cfg = self.cfg
        if cfg.scene_centre is None or cfg.scene_phys_bounds is None or cfg.sample_res is None:                    # :94-96
            raise ValueError("build_scene_model needs cfg.scene_centre, cfg.scene_phys_bounds and cfg.sample_res")
        intrinsics = self.intrinsics
        loader = d2r_dataloader(cfg, self.ctx)
        if raw_data is None:
            rgbs, depths, raw_cam_poses = loader.load_rgbds()
        else:
            rgbs, depths, raw_cam_poses = (_np(a) for a in raw_data)
            loader.rgb_data, loader.depth_data, loader.T_WC_data = rgbs, depths, np.asarray(raw_cam_poses, np.float32).reshape(-1, 4, 4)
            loader.size = len(depths)
        self.out_scene_bound_masks = loader.remove_background(intrinsics, cfg.scene_phys_bounds, use_cache=cfg.use_cache_dynamic_masks)

        self.depths_gt = np.stack([_np(depths[i]) for i in cfg.render_cam_pose_idx])                              # :117-118

        if cfg.use_cache_segs:                                                                                    # :121-137
            masks = segmentation.load_cached_masks(self.data_dir, len(depths))
        elif self.segmentor is not None:
            raw_masks = np.asarray(_np(self.segmentor(rgbs, depths)), np.uint8)
            masks = segmentation.refine_masks(raw_masks, depths, loader.T_WC_data, intrinsics, self.out_scene_bound_masks,
                                              cfg.scene_centre, self.data_dir, ctx=self.ctx)
        elif self.proposer is not None:
            # segment_associate with every frame associated (XMem_infer.py:199-236): proposals on the upright first frame, the
            # rule of DESIGN.md section 2h on the GPU, the tracker over all frames, then the same refinement
            rgbs_np = _np(rgbs)
            first = np.rot90(rgbs_np[0], 1)
            inside = np.rot90(_np(self.out_scene_bound_masks[0]) == 0)
            if isinstance(self.proposer, str):             # "geometric": frame 0's depth in sensor orientation, the masks turned as the frame is
                up = -np.asarray(physics_utils.GRAVITY_DIRECTION, np.float64)
                proposals = np.rot90(segmentation.propose_masks(depths[0], loader.T_WC_data[0], intrinsics, cfg.scene_phys_bounds, up=up,
                                                                ctx=self.ctx)[0], 1, axes=(1, 2))
            else:
                proposals = self.proposer(first)
            labels0 = np.rot90(segmentation.proposals_to_labels(proposals, inside, ctx=self.ctx), 3)
            if isinstance(self.tracker, str):              # "geometric"
                raw_masks = segmentation.track_labels(depths, loader.T_WC_data, intrinsics, np.ascontiguousarray(labels0),
                                                      cfg.scene_phys_bounds, ctx=self.ctx)
            else:
                raw_masks = np.asarray(_np(self.tracker(rgbs, np.ascontiguousarray(labels0))), np.uint8)
            if raw_masks.shape != rgbs_np.shape[:3]:
                raise ValueError(f"tracker returned label images of shape {raw_masks.shape}, expected {rgbs_np.shape[:3]}")
            masks = segmentation.refine_masks(raw_masks, depths, loader.T_WC_data, intrinsics, self.out_scene_bound_masks,
                                              cfg.scene_centre, self.data_dir, ctx=self.ctx)
        else:
            raise RuntimeError("build_scene_model: running SAM and XMem is out of scope; either set use_cache_segs and provide "
                               "XMem_masks/rgb_%04d.png in data_dir, or pass segmentor=callable(rgbs, depths) -> uint8 [N,H,W] "
                               "raw label images to the engine, or pass proposer= (image -> mask proposals) and tracker= "
                               "(frames, first label image -> label images) and let the engine build the first label image")

        _, num_objs, self.label_counts = segmentation.label_census(masks, ctx=self.ctx)                           # :139-144
        if num_objs == 0:
            raise ValueError("build_scene_model: the masks hold no label below 255: every pixel is outside the scene bounds")

        if cfg.use_cache_cam_poses:                                                                               # :146-151
            opt_cam_poses = np.load(os.path.join(self.data_dir, "opt_cam_poses.npy"))
        elif cfg.use_vis_pcds or cfg.vis_backend == "tsdf":
            opt_cam_poses = np.asarray(loader.T_WC_data)           # the ablation renders clouds, the TSDF backend volumes: no NeRF, no pose optimisation
            if cfg.cam_pose_refine == "tsdf":                      # ... but each frame tracked against the volume fused so far
                from . import cam_pose_opt
                opt_cam_poses, reports = cam_pose_opt.refine_cam_poses(depths, opt_cam_poses, intrinsics, self.out_scene_bound_masks,
                                                                       cfg.scene_phys_bounds, ctx=self.ctx)
                with open(os.path.join(self.data_dir, "cam_pose_refine.json"), "w") as f:
                    json.dump(reports, f, indent=1)
            np.save(os.path.join(self.data_dir, "opt_cam_poses.npy"), opt_cam_poses)
        else:
            raise NotImplementedError("build_scene_model: optimised camera poses come out of NeRF training, which is not implemented; "
                                      "set use_cache_cam_poses (opt_cam_poses.npy in data_dir) or use_vis_pcds")
        opt_cam_poses = [torch.tensor(pose) for pose in opt_cam_poses]

        if cfg.lazy_phys_mods:                                                                                    # :153-160
            phys_models, init_poses = [None] * num_objs, [None] * num_objs
        else:
            phys_models, init_poses = physics_utils.get_phys_models(
                depths, opt_cam_poses, intrinsics, masks, num_objs, cfg.scene_phys_bounds, save_dir=os.path.join(self.data_dir, "phys_mods/"),
                vis=not cfg.use_cache_phys, use_cache=cfg.use_cache_phys, use_phys_tsdf=cfg.use_phys_tsdf, ctx=self.ctx,
                phys_backend=cfg.phys_backend)

        captions_path = os.path.join(self.data_dir, "captions.json")                                              # :83, :162-164
        given = captions is not None
        thumbnails = [None] * num_objs
        if not given and self.captioner is not None:               # :162-164, caption.py:55-169 with the image work on the GPU
            from . import caption
            captions, thumbnails = caption.caption_objs(
                num_objs, rgbs, masks, self.lang_model, self.out_scene_bound_masks, self.topdown, multi_view=cfg.multi_view_captions,
                single_view_idx=cfg.single_view_idx, ctx=self.ctx, captioner=self.captioner, cache_path=captions_path,
                read_cache=cfg.use_cache_captions)
        elif not given:
            if not os.path.exists(captions_path):
                raise RuntimeError(f"build_scene_model: captioning models are out of scope; pass captions=[...] or provide {captions_path}, "
                                   "or pass captioner=callable(list of thumbnails) -> list of captions to the engine")
            with open(captions_path) as f:
                captions = json.load(f)
        captions = list(captions)
        if len(captions) != num_objs or captions[0] != "__background__":
            raise ValueError(f"build_scene_model: {len(captions)} captions {captions} for {num_objs} objects (labels 0 .. {num_objs - 1}); "
                             'there must be one per object and the first must be "__background__"')
        if given and not cfg.use_cache_captions:                   # the reference's captioner leaves its result there (caption.py:166-167)
            with open(captions_path, "w") as f:
                json.dump(captions, f)

        vis_models = [None] * num_objs                             # created lazily once the task is known (:167-168)
        objs = [ObjectModel(captions[k], vis_models[k], phys_models[k], init_poses[k], thumbnails[k], k) for k in range(num_objs)]
        self.scene_model = SceneModel(cfg.scene_centre, objs, objs[0], rgbs, depths, opt_cam_poses, intrinsics, masks,
                                      cfg.scene_phys_bounds, cfg.scene_type)

    def determine_movable_obj(self, user_instr):
        """reference :179-193 -> (movable_obj, movable_idx)"""
        obj_captions = [obj.name for obj in self.scene_model.objs]
        movable_idx = self.lang_model.get_movable_obj_idx(user_instr, obj_captions)
        return self.scene_model.objs[movable_idx], movable_idx

    def determine_relevant_objs(self, norm_caption, movable_obj_idx):
        """reference :195-214: the objects that are not distractors."""
        obj_captions = [obj.name for obj in self.scene_model.objs]
        relevant_idxs = self.lang_model.get_relevant_obj_idxs(norm_caption, obj_captions, movable_obj_idx)
        if len(relevant_idxs) == 0:
            raise RuntimeError("Error: None of the captioned objects were determined to be relevant.")
        return [self.scene_model.objs[idx] for idx in relevant_idxs]

    def interpret_user_instr(self, user_instr, goal_caption=None, norm_captions=None):
        """reference dream2real.py:216-280 -> TaskModel."""
        from .scene_model import TaskModel
        cfg = self.cfg
        if self.scene_model is None:
            raise RuntimeError("Must call build_scene_model() first before receiving user instructions")
        if self.lang_model is None:
            raise RuntimeError("interpret_user_instr needs lang_model= (e.g. CachedLangModel(path)): no LLM is called from here")
        if goal_caption is None:
            goal_caption, norm_caption = self.lang_model.parse_instr(user_instr)
            norm_captions = [norm_caption]
        movable_obj, movable_obj_idx = self.determine_movable_obj(user_instr)
        relevant_objs = self.determine_relevant_objs(goal_caption, movable_obj_idx)

        # before the visual models, as in the reference (:244-250)
        if cfg.lazy_phys_mods:
            [bground_phys, movable_phys], [bground_init_pose, movable_init_pose] = TaskModel.create_lazy_phys_mods(
                self.scene_model, movable_obj, cfg.scene_phys_bounds, save_dir=os.path.join(self.data_dir, "phys_mod/"), embodied=cfg.embodied,
                vis=False, use_cache=cfg.use_cache_phys, use_phys_tsdf=cfg.use_phys_tsdf, use_vis_pcds=cfg.use_vis_pcds,
                single_view_idx=cfg.single_view_idx, ctx=self.ctx, phys_backend=cfg.phys_backend)

        movable_obj.vis_model = TaskModel.create_movable_vis_model(
            self.scene_model, movable_obj, self.out_scene_bound_masks, os.path.join(self.data_dir, "movable_vis_mod/"),
            use_vis_pcds=cfg.use_vis_pcds, pcds_type=cfg.pcds_type, single_view_idx=cfg.single_view_idx, use_cache=cfg.use_cache_vis,
            data_dir=self.data_dir, ctx=self.ctx, vis_backend=cfg.vis_backend)
        task_bground_obj, task_bground_masks = TaskModel.create_task_bground_obj(
            self.scene_model, movable_obj, relevant_objs, self.out_scene_bound_masks, os.path.join(self.data_dir, "task_bground_vis_mod/"),
            use_vis_pcds=cfg.use_vis_pcds, pcds_type=cfg.pcds_type, single_view_idx=cfg.single_view_idx,
            render_distractors=cfg.render_distractors, use_cache=cfg.use_cache_vis, data_dir=self.data_dir, ctx=self.ctx,
            vis_backend=cfg.vis_backend)

        if cfg.lazy_phys_mods:                                                                                    # :274-277
            movable_obj.phys_model = movable_phys
            movable_obj.pose = movable_init_pose
            task_bground_obj.phys_model = bground_phys

        return TaskModel(user_instr, goal_caption, norm_captions, self.scene_model, movable_obj, task_bground_obj, task_bground_masks,
                         self.topdown)

    def _vis_view(self, task_model):
        """The view of the two pictures: the first render view's OpenCV pose, the scene's intrinsics scaled from the sensor's
        width x height to cfg.resolution (pixel centres at whole numbers: c' = (c + 0.5) s - 0.5)."""
        from . import _lib, geometry_utils
        from .virtual_cam_pose_sample import get_virtual_cam_poses
        cfg = self.cfg
        W, H = cfg.resolution if cfg.resolution is not None else combined_rendering.renderer.resolution
        K = np.asarray(task_model.scene_model.intrinsics, np.float64)
        sx, sy = W / cfg.width, H / cfg.height
        view = _lib.PcdView(int(W), int(H), K[0, 0] * sx, K[1, 1] * sy, (K[0, 2] + 0.5) * sx - 0.5, (K[1, 2] + 0.5) * sy - 0.5, 1.0,
                            geometry_utils.VIS_NEAR)
        return view, get_virtual_cam_poses(task_model, list(cfg.render_cam_pose_idx))[0]

    def _vis_best_pose(self, task_model, best_pose, pose_batch, pose_scores):
        """reference dream2real.py:360-400 with tsdf_vis: cost_volume.png (not with use_vis_pcds, as there) and best_pose_vis.png
        into data_dir, rotated like best_render.png; rank 0 writes."""
        from . import _lib, geometry_utils
        from .dist import process_rank
        if process_rank() != 0:
            return
        cfg = self.cfg
        bground_geoms = [os.path.join(self.data_dir, "phys_mod/mesh_concave_0.obj")]
        movable_geom = os.path.join(self.data_dir, "phys_mod/mesh_concave_1.obj")
        for path in bground_geoms + [movable_geom]:
            if not os.path.exists(path):
                raise FileNotFoundError(f"dream_best_pose(vis_cost_vol=True) draws {path}, which is missing")
        view, cam_pose = self._vis_view(task_model)
        rot = lambda frame: np.ascontiguousarray(np.rot90(frame, k=1, axes=(0, 1)))
        if not cfg.use_vis_pcds:
            frame = geometry_utils.vis_cost_volume(pose_scores, list(cfg.sample_res), pose_batch, bground_geoms, ctx=self.ctx, view=view,
                                                   cam_pose=cam_pose)
            _lib.png_write(rot(frame), os.path.join(self.data_dir, "cost_volume.png"))
        frame = geometry_utils.vis_best_pose(best_pose, bground_geoms, movable_geom, task_model.movable_obj.pose, ctx=self.ctx, view=view,
                                             cam_pose=cam_pose)
        _lib.png_write(rot(frame), os.path.join(self.data_dir, "best_pose_vis.png"))

    def dream_best_pose(self, task_model, vis_cost_vol=False):
        """-> (best_pose [4,4], pose_batch [N,16], pose_scores [N]) as torch tensors; writes goal_pose.txt,
        pose_batch.txt, pose_scores.txt (and best_render.png, cb_render/*.png through the path) into data_dir.
        reference dream2real.py:286-358.  vis_cost_vol (the reference's :360-400, off by default here: nothing else is
        written without it): also cost_volume.png and best_pose_vis.png from phys_mod/mesh_concave_{0,1}.obj, on the cached
        branch too; a missing mesh file is a FileNotFoundError naming it."""
        import torch
        cfg = self.cfg
        unsupcol_check = None
        if cfg.use_phys and not cfg.use_cache_renders:                                           # :304-323
            unsupcol_check, static_obj_handles, movable_handles = physics_utils.create_unsupcol_check(
                self.ctx, task_model, cfg.sample_res, cfg.embodied, lazy_phys_mods=cfg.lazy_phys_mods)
            self.static_phys_handles = static_obj_handles
            self.movable_phys_handle = movable_handles[0]
            # the reference composes the check with a PyBullet shutdown when it is not embodied; here the GPU shapes
            # are released the same way, after the check has run
            release = lambda pose_batch, task_model, valid_so_far: (unsupcol_check.shapes.close(), valid_so_far)[1]
            phys_check = unsupcol_check if cfg.embodied else compose_checks([unsupcol_check, release])
        else:                                                                                    # :324-326
            phys_check = lambda pose_batch, task_model, valid_so_far: torch.ones(len(pose_batch), dtype=torch.bool)

        if cfg.vis_backend == "tsdf" and not cfg.use_cache_goal_pose:
            from .tsdf_visual_model import TsdfRenderer
            self.renderer = TsdfRenderer(self.ctx)        # 336 x 336 through INTRINSICS_CLIP_VIEW, as the point-cloud renderer
        elif cfg.use_vis_pcds and not cfg.use_cache_goal_pose:                                   # :329-332
            from .pcd_visual_model import PointCloudRenderer
            self.renderer = PointCloudRenderer(self.ctx)
        else:
            self.renderer = combined_rendering.renderer(self.data_dir, task_model, resolution=cfg.resolution)

        if cfg.use_cache_goal_pose:                                                              # :335-341
            best_pose = torch.tensor(np.loadtxt(os.path.join(self.data_dir, "goal_pose.txt"))).float()
            pose_batch = torch.tensor(np.loadtxt(os.path.join(self.data_dir, "pose_batch.txt"))).float()
            pose_scores = torch.tensor(np.loadtxt(os.path.join(self.data_dir, "pose_scores.txt"))).float()
            if vis_cost_vol:
                self._vis_best_pose(task_model, best_pose, pose_batch, pose_scores)
            return best_pose, pose_batch, pose_scores
        best_pose, pose_batch, pose_scores = clip_scoring.optimise_pose_grid(                    # :343-355
            self.renderer, self.depths_gt, list(cfg.render_cam_pose_idx), task_model, self.data_dir,
            sample_res=list(cfg.sample_res), phys_check=phys_check, use_templates=False, scene_type=cfg.scene_type,
            use_vis_pcds=cfg.use_vis_pcds, use_cache_renders=cfg.use_cache_renders, smoothing=cfg.spatial_smoothing,
            physics_only=cfg.physics_only, scorer=self.scorer, text_embeds=self.text_embeds, text_encoder=self.text_encoder,
            tokenizer=self.tokenizer, save_renders=cfg.save_renders)
        from .dist import process_rank
        if process_rank() == 0:        # pose-sharded runs: every rank holds the same result, one of them writes it
            clip_scoring.save_pose_outputs(self.data_dir, best_pose, pose_batch, pose_scores)     # :356-358
        if vis_cost_vol:
            self._vis_best_pose(task_model, best_pose, pose_batch, pose_scores)
        return best_pose, pose_batch, pose_scores
