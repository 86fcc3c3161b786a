"""A scan folder and a settings file in, the best pose out: the three calls of ImaginationEngine.
    python examples/scene_to_pose.py configs/shopping/pcd.json data/shopping "put the apple in the bowl" clip_dir [--vis] [--vis-backend tsdf] [--refine-poses] [--dump-thumbnails DIR] [--proposals FILE.npy --tracked FILE.npy | --proposals FILE.npy --geometric-tracker | --geometric-proposer] [--clip-captioner]
--vis also writes best_pose_vis.png (and, without use_vis_pcds, cost_volume.png) into the folder.
--vis-backend tsdf renders the candidates from colour-TSDF volumes fused from the scan instead of the settings
file's visual model (NeRF snapshots, or point clouds with use_vis_pcds, which it switches off).
--refine-poses refines each frame's camera pose against the TSDF volume fused so far (it needs use_vis_pcds or
--vis-backend tsdf, and no use_cache_cam_poses) and writes cam_pose_refine.json beside opt_cam_poses.npy.
--dump-thumbnails DIR writes the objects' captioning thumbnails as DIR/obj_<object>_<k>.png, to caption them elsewhere.
--proposals FILE.npy --tracked FILE.npy stand in for the two segmentation models: the mask generator's recorded proposals, bool [M,W,H]
for the first frame turned upright, and the tracker's recorded raw label images, uint8 [N,H,W]; the engine builds the first label image
between them instead of reading XMem_masks/.
--geometric-tracker in place of --tracked: the first label image is carried through the scan by depth and pose on the GPU (DESIGN.md
section 2k), no tracking network and no recording of one.
--geometric-proposer: no segmentation model and no recording at all, for a table-top scene (scene_type 0 or 3): the proposals are
what stands above the support plane in the first frame's depth and the geometric tracker carries them.
--clip-captioner: no captioning model and no captions.json: the objects are named from the package's vocabulary of object names by the
CLIP checkpoint's own towers, the thumbnails never leaving the GPU; captions.json and caption_scores.json are
written.  With --geometric-proposer only lang_cache.json is still read.
The folder holds poses.txt, images/, depth/, XMem_masks/ (use_cache_segs), captions.json and lang_cache.json (a
CachedLangModel file); clip_dir holds a CLIP checkpoint: model.safetensors, vocab.json, merges.txt."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dream2real_amd import engine
from dream2real_amd.clip_model import load_clip_safetensors
from dream2real_amd.dream2real import CachedLangModel, ImaginationEngine, PathConfig
from dream2real_amd.tokenizer import ClipBpeTokenizer

argv, dump_dir = sys.argv[1:], None
if "--dump-thumbnails" in argv:
    at = argv.index("--dump-thumbnails")
    dump_dir = argv[at + 1]
    del argv[at:at + 2]
backend = {}
if "--vis-backend" in argv:
    at = argv.index("--vis-backend")
    backend = dict(vis_backend=argv[at + 1])
    if argv[at + 1] == "tsdf":
        backend.update(use_vis_pcds=False, pcds_type=None)
    del argv[at:at + 2]
if "--refine-poses" in argv:
    argv.remove("--refine-poses")
    backend.update(cam_pose_refine="tsdf")
recorded = {}
for flag in ("--proposals", "--tracked"):
    if flag in argv:
        at = argv.index(flag)
        recorded[flag] = argv[at + 1]
        del argv[at:at + 2]
geometric = "--geometric-tracker" in argv
if geometric:
    argv.remove("--geometric-tracker")
if geometric and "--tracked" in recorded:
    sys.exit("--geometric-tracker stands in place of --tracked")
if ("--proposals" in recorded) != (geometric or "--tracked" in recorded):
    sys.exit("--proposals comes with --tracked or --geometric-tracker")
geometric_proposer = "--geometric-proposer" in argv
if geometric_proposer:
    argv.remove("--geometric-proposer")
    if recorded or geometric:
        sys.exit("--geometric-proposer stands alone: it implies the geometric tracker and takes no recorded proposals")
if "--clip-captioner" in argv:
    argv.remove("--clip-captioner")
    models_captioner = dict(captioner="clip")
else:
    models_captioner = {}
vis = "--vis" in argv
config_file, data_dir, user_instr, clip_dir = [a for a in argv if a != "--vis"][:4]
cfg = PathConfig.from_json(config_file, data_dir, use_cache_segs=not (recorded or geometric_proposer), phys_backend="tsdf", **backend)
models = {}
if recorded:
    import numpy as np
    models = dict(proposer=lambda image: np.load(recorded["--proposals"]),
                  tracker="geometric" if geometric else lambda frames, labels0: np.load(recorded["--tracked"]))
if geometric_proposer:
    models = dict(proposer="geometric", tracker="geometric")
models.update(models_captioner)
ctx = engine.Context(0)
clip_cfg, state = load_clip_safetensors(os.path.join(clip_dir, "model.safetensors"))
imagination = ImaginationEngine(cfg, ctx, engine.ClipScorer(ctx, clip_cfg, state),
                                text_encoder=engine.TextEncoder(ctx, clip_cfg, state),
                                tokenizer=ClipBpeTokenizer.from_files(os.path.join(clip_dir, "vocab.json"), os.path.join(clip_dir, "merges.txt"),
                                                                     context_length=clip_cfg["ctx"]),
                                lang_model=CachedLangModel(os.path.join(data_dir, "lang_cache.json")), **models)
imagination.build_scene_model()
if dump_dir is not None:
    from dream2real_amd import _lib, caption
    scene = imagination.scene_model
    os.makedirs(dump_dir, exist_ok=True)
    thumbnails = caption.object_thumbnails(len(scene.objs), scene.rgbs, scene.masks, imagination.out_scene_bound_masks, imagination.topdown,
                                           cfg.multi_view_captions, cfg.single_view_idx, ctx=ctx)
    for obj_idx, obj_thumbnails in enumerate(thumbnails, start=1):
        for k, image in enumerate(obj_thumbnails):
            _lib.png_write(image, os.path.join(dump_dir, "obj_%03d_%02d.png" % (obj_idx, k)))
task_model = imagination.interpret_user_instr(user_instr)
best_pose, pose_batch, pose_scores = imagination.dream_best_pose(task_model, vis_cost_vol=vis)
print(best_pose)
