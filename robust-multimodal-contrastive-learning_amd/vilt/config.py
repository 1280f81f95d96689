"""Plain-dict restatement of the reference's sacred config (vilt/config.py:24-116) with the
``task_moco`` overrides (:128-164).  sacred itself is out of scope; the KEYS and DEFAULTS are part
of the drop-in boundary."""


def _loss_names(d):
    ret = {"moco": 0, "barlowtwins": 0, "itm": 0, "mlm": 0, "mpp": 0, "vqa": 0, "nlvr2": 0, "irtr": 0,
           "irtr_attacked": 0, "nlvr2_attacked": 0, "vqa_attacked": 0}
    ret.update(d)
    return ret


# Not reference keys: the PGD threat model of the image attack (attack/pgd_attack_vilt.py ThreatModel, DESIGN.md "PGD threat models").
# The defaults are the reference's loop, bit for bit: L-inf ball, step g / max|g|, delta_0 = 0, no pixel box.
#   adv_norm_img          "linf" | "l2"
#   adv_step_rule_img     "normalised" | "sign"   (ignored for "l2": the step is g / ||g||_2)
#   adv_random_start_img  bool
#   adv_pixel_box_img     None | (lo, hi)         ((-1.0, 1.0) for the pixelbert normalisation)
#   adv_seed_img          int                     mixed with the engine's pass counter for each step's random start
# Unknown values raise a ValueError when the attacker is built.
ADV_IMG_THREAT = dict(adv_norm_img="linf", adv_step_rule_img="normalised", adv_random_start_img=False, adv_pixel_box_img=None, adv_seed_img=0)


def default_config(**over):
    cfg = dict(
        exp_name="vilt", seed=0, loss_names=_loss_names({"itm": 1, "mlm": 1}), batch_size=4096,
        image_size=384, max_image_len=-1, patch_size=32, draw_false_image=1, image_only=False,
        vqav2_label_size=3129, max_text_len=40, tokenizer="bert-base-uncased", vocab_size=30522,
        whole_word_masking=False, mlm_prob=0.15, draw_false_text=0,
        vit="vit_base_patch32_384", hidden_size=768, num_heads=12, num_layers=12, mlp_ratio=4, drop_rate=0.1,
        optim_type="adamw", learning_rate=1e-4, weight_decay=0.01, decay_power=1, max_epoch=100, max_steps=25000,
        warmup_steps=2500, end_lr=0, lr_mult=1,
        get_recall_metric=False, resume_from="", fast_dev_run=False, val_check_interval=1.0, test_only=False,
        data_root="", log_dir="result", per_gpu_batchsize=0, num_gpus=1, num_nodes=1, load_path="",
        num_workers=8, precision=16,
        # not reference keys.  skip_nonfinite_steps: drop an optimizer step whose gradient holds a NaN / inf (what the GradScaler of the
        # reference's precision=16 does); gradient_clip_val: Lightning's Trainer argument of that name (its default 0 = off; run.py does
        # not set it).  Either one switches FusedAdamW to the guarded step (DESIGN.md "Guarded step and resumable state")
        skip_nonfinite_steps=False, gradient_clip_val=0.0,
    )
    cfg.update(over)
    return cfg


def task_moco(**over):
    cfg = default_config(
        exp_name="moco", Multimodal=True, num_negative=65536, momentum=0.999, temperature=0.07,
        augmentation=False, text_view=False, image_view=False, loss_names=_loss_names({"moco": 1}),
        batch_size=128, max_epoch=1, max_image_len=200, test_only=False,
        adv_steps_img=5, adv_lr_img=0.05, adv_max_norm_img=0.005, **ADV_IMG_THREAT,
        n_candidates=5, max_loops=10, sim_thred=0.5, cos_sim=True, synonym="cos_sim",
        # reference config.py:161-162; the word-level text attack is active when `tokenizer` is a LOCAL vocab path (or an
        # object) and embedding_path exists - with the hub name "bert-base-uncased" it runs at token level
        embedding_path="../attack/counter-fitted-vectors.txt", sim_path="../attack/cos_sim_counter_fitting.npy", stopwords=None,
        TSNE_vizualisation=False, img_save_path="",
    )
    cfg.update(over)
    return cfg


def task_barlowtwins(**over):
    """reference config.py:166-199: the Barlow-Twins variant of the contrastive pre-training.
    barlowtwins_dims: widths of BarlowTwinsHead - the reference hard-codes [8192, 8192], 8192 (vilt_module.py:115)."""
    cfg = default_config(
        exp_name="barlowtwins", Multimodal=True, augmentation=False, text_view=False, image_view=False,
        loss_names=_loss_names({"barlowtwins": 1}), adv_lr=0.0051, batch_size=128, max_epoch=1, max_image_len=200, test_only=False,
        adv_steps_img=5, adv_lr_img=0.05, adv_max_norm_img=0.005, **ADV_IMG_THREAT,
        n_candidates=5, max_loops=10, sim_thred=0.5, cos_sim=True, synonym="cos_sim",
        embedding_path="../attack/counter-fitted-vectors.txt", sim_path="../attack/cos_sim_counter_fitting.npy", stopwords=None,
        TSNE_vizualisation=False, img_save_path="", barlowtwins_dims=(8192, 8192, 8192),
    )
    cfg.update(over)
    return cfg


def task_finetune_vqa(**over):
    """reference config.py:289-302: VQAv2 fine-tuning (vqa_classifier + soft-target BCE).  max_steps None as in the reference:
    set_schedule then needs it from the caller."""
    cfg = default_config(
        exp_name="finetune_vqa", datasets=["vqa"], loss_names=_loss_names({"vqa": 1}), batch_size=256, max_epoch=10,
        max_steps=None, warmup_steps=0.1, draw_false_image=0, learning_rate=1e-4, val_check_interval=0.1, lr_mult=10,
    )
    cfg.update(over)
    return cfg


def task_finetune_vqa_randaug(**over):
    """reference config.py:305-317: as task_finetune_vqa with the RandAugment train transform (vilt/transforms/randaug.py)."""
    cfg = task_finetune_vqa(exp_name="finetune_vqa_randaug", train_transform_keys=["pixelbert_randaug"])
    cfg.update(over)
    return cfg


def task_finetune_vqa_randaug_attacked(**over):
    """reference config.py:319-348: adversarial VQAv2 fine-tuning.  Both views default to False as in the reference, which then fails
    in compute_vqa_attack; here the module refuses that at construction (ValueError): pass image_view=True (PGD on the image) and / or
    text_view=True (GreedyAttack_vqa, word level: `tokenizer` must then be a local vocabulary path and `embedding_path` a local file)."""
    cfg = default_config(
        exp_name="finetune_vqa_randaug_attacked", datasets=["vqa"], train_transform_keys=["pixelbert_randaug"],
        loss_names=_loss_names({"vqa_attacked": 1}), batch_size=128, max_epoch=10, max_steps=None, warmup_steps=0.1,
        draw_false_image=0, learning_rate=1e-4, val_check_interval=0.1, lr_mult=10,
        text_view=False, image_view=False, adv_steps_img=5, adv_lr_img=0.05, adv_max_norm_img=0.005, **ADV_IMG_THREAT,
        n_candidates=5, max_loops=10, sim_thred=0.5, cos_sim=True, synonym="cos_sim",
        embedding_path="../attack/counter-fitted-vectors.txt", sim_path="../attack/cos_sim_counter_fitting.npy",
    )
    cfg.update(over)
    return cfg


def task_finetune_nlvr2(**over):
    """reference config.py:234-243: NLVR2 fine-tuning (3-row token_type_embeddings, nlvr2_classifier + cross-entropy).  max_steps None as
    in the reference: set_schedule then needs it from the caller.  nlvr2_pair_pass (not a reference key, default True): the two images
    of a pair run as ONE encoder pass of 2B sequences; False runs the reference's two infer calls (DESIGN.md "NLVR2 fine-tuning")."""
    cfg = default_config(
        exp_name="finetune_nlvr2", datasets=["nlvr2"], loss_names=_loss_names({"nlvr2": 1}), batch_size=128, max_epoch=10,
        max_steps=None, warmup_steps=0.1, draw_false_image=0, learning_rate=1e-4, nlvr2_pair_pass=True,
    )
    cfg.update(over)
    return cfg


def task_finetune_nlvr2_randaug(**over):
    """reference config.py:245-256: as task_finetune_nlvr2 with the RandAugment train transform (vilt/transforms/randaug.py)."""
    cfg = task_finetune_nlvr2(exp_name="finetune_nlvr2_randaug", train_transform_keys=["pixelbert_randaug"])
    cfg.update(over)
    return cfg


def task_finetune_nlvr2_randaug_attacked(**over):
    """reference config.py:258-288: adversarial NLVR2 fine-tuning.  Both views default to False as in the reference, which then fails
    (no nlvr2_attacked_loss); here the module refuses that at construction (ValueError): pass image_view=True (PGD on the images
    selected by attack_idx) and / or text_view=True (GreedyAttack_nlvr2, word level: `tokenizer` must then be a local vocabulary path and
    `embedding_path` a local file)."""
    cfg = default_config(
        exp_name="finetune_nlvr2_randaug_attacked", datasets=["nlvr2"], train_transform_keys=["pixelbert_randaug"],
        loss_names=_loss_names({"nlvr2_attacked": 1}), batch_size=128, max_epoch=10, max_steps=None, warmup_steps=0.1,
        draw_false_image=0, learning_rate=1e-4, test_only=False, text_view=False, image_view=False,
        adv_steps_img=5, adv_lr_img=0.05, adv_max_norm_img=0.005, **ADV_IMG_THREAT, attack_idx=[True, True],
        n_candidates=5, max_loops=10, sim_thred=0.5, cos_sim=True, synonym="cos_sim",
        embedding_path="../attack/counter-fitted-vectors.txt", sim_path="../attack/cos_sim_counter_fitting.npy", nlvr2_pair_pass=True,
    )
    cfg.update(over)
    return cfg


def task_finetune_irtr_coco(**over):
    """reference config.py:349-360: image-text retrieval fine-tuning on COCO (itm + irtr: rank_output on row 1 of the ITM head, 15 false
    captions per image, recalls at every validation end).  max_steps None as in the reference: set_schedule then needs it from the caller."""
    cfg = default_config(
        exp_name="finetune_irtr_coco", datasets=["coco"], loss_names=_loss_names({"itm": 0.5, "irtr": 1}), batch_size=256, max_epoch=128,
        max_steps=None, warmup_steps=0.1, get_recall_metric=True, draw_false_text=15, learning_rate=1e-4,
    )
    cfg.update(over)
    return cfg


def task_finetune_irtr_coco_randaug(**over):
    """reference config.py:363-375 (the RandAugment train transform: vilt/transforms/randaug.py)."""
    cfg = default_config(
        exp_name="finetune_irtr_coco_randaug", datasets=["coco"], train_transform_keys=["pixelbert_randaug"],
        loss_names=_loss_names({"itm": 0.5, "irtr": 1}), batch_size=128, max_epoch=2, max_steps=None, warmup_steps=0.1,
        get_recall_metric=True, draw_false_text=15, learning_rate=1e-4,
    )
    cfg.update(over)
    return cfg


def task_finetune_irtr_f30k(**over):
    """reference config.py:408-419: image-text retrieval fine-tuning on Flickr30k."""
    cfg = default_config(
        exp_name="finetune_irtr_f30k", datasets=["f30k"], loss_names=_loss_names({"itm": 0.5, "irtr": 1}), batch_size=128, max_epoch=10,
        max_steps=None, warmup_steps=0.1, get_recall_metric=True, draw_false_text=15, learning_rate=1e-4,
    )
    cfg.update(over)
    return cfg


def task_finetune_irtr_f30k_randaug(**over):
    """reference config.py:422-434 (the RandAugment train transform: vilt/transforms/randaug.py)."""
    cfg = default_config(
        exp_name="finetune_irtr_f30k_randaug", datasets=["f30k"], train_transform_keys=["pixelbert_randaug"],
        loss_names=_loss_names({"itm": 0.5, "irtr": 1}), batch_size=128, max_epoch=10, max_steps=None, warmup_steps=0.1,
        get_recall_metric=True, draw_false_text=15, learning_rate=1e-4,
    )
    cfg.update(over)
    return cfg


def task_mlm_itm(**over):
    """reference config.py:202-209: ViLT pre-training, masked language modelling + image-text matching (the objective that produced
    vilt_200k_mlm_itm.ckpt).  The reference's own `datasets` line keeps COCO only (the four-dataset list is commented out there)."""
    cfg = default_config(
        exp_name="mlm_itm", datasets=["coco"], loss_names=_loss_names({"itm": 1, "mlm": 1}), batch_size=4096, max_epoch=10,
        max_image_len=200,
    )
    cfg.update(over)
    return cfg


def task_mlm_itm_mpp(**over):
    """reference config.py:223-230: ViLT pre-training with masked patch prediction on top of MLM and ITM."""
    cfg = default_config(
        exp_name="mlm_itm_mpp", datasets=["coco", "vg", "sbu", "gcc"], loss_names=_loss_names({"itm": 1, "mlm": 1, "mpp": 1}),
        batch_size=4096, max_epoch=10, max_image_len=200,
    )
    cfg.update(over)
    return cfg


def task_mlm_itm_randaug(**over):
    """reference config.py:212-220 (the RandAugment train transform: vilt/transforms/randaug.py)."""
    cfg = default_config(
        exp_name="mlm_itm_randaug", datasets=["coco", "vg", "sbu", "gcc"], train_transform_keys=["pixelbert_randaug"],
        loss_names=_loss_names({"itm": 1, "mlm": 1}), batch_size=4096, max_epoch=10, max_image_len=200,
    )
    cfg.update(over)
    return cfg
