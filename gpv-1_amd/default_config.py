"""Built-in configuration tree of the drivers (gpv1_amd.train_distr, gpv1_amd.inference).

Same schema as the Hydra tree the reference's drivers read (``model`` / ``model.losses`` are what ``GPV(cfg.model)`` consumes,
``training`` what the training driver consumes, ``eval`` what the inference harness consumes); ``${...}`` references are
resolved by gpv1_amd.config.  Pass ``--config some.yaml`` to the drivers to load a YAML file instead -- the reference's own
``configs/exp/gpv.yaml`` loads as it is.  Hydra ``defaults:`` groups (datasets / tasks) are data-loading configuration and
are not reproduced (out of scope).
"""
import copy

_TREE = {'exp_name': 'default',
 'output_dir': 'gpv_output',
 'exp_dir': '${output_dir}/${exp_name}',
 'tb_dir': '${exp_dir}/tb_logs',
 'ckpt_dir': '${exp_dir}/ckpts',
 'data_dir': 'gpv_data',
 'gpu': 0,
 'num_nodes': 1,
 'ngpus_per_node': 8,
 'world_size': None,
 'rank': 0,
 'workers': '${training.num_workers}',
 'batch_size': '${training.batch_size}',
 'dist_backend': 'nccl',
 'dist_url': 'tcp://localhost:10001',
 'multiprocessing_distributed': True,
 'model': {'pretr_detr': '${data_dir}/detr/detr_coco_sce.pth',
           'vocab': '${data_dir}/learning_phase_data/vocab/vocab.json',
           'vocab_embed': '${data_dir}/learning_phase_data/vocab/vocab_embed.npy',
           'max_pos_enc_len': 30,
           'max_text_len': 20,
           'answer_head': None,
           'answering_type': 'generation',
           'hidden_dim': 768,
           'roi_head': True,
           'relevance_conditioning': True,
           'detr': {'num_queries': 100,
                    'num_classes': 1,
                    'hidden_dim': 256,
                    'nheads': 8,
                    'num_encoder_layers': 6,
                    'num_decoder_layers': 6,
                    'backbone': 'resnet50',
                    'lr_backbone': 1e-05,
                    'position_embedding': 'sine',
                    'masks': False,
                    'dilation': False,
                    'dropout': 0.1,
                    'dim_feedforward': 2048,
                    'pre_norm': False,
                    'aux_loss': False,
                    'frozenbatchnorm': True,
                    'last_layer_only': True},
           'detr_joiner': {'detr_dim': 2304, 'out_dim': 768},
           'bert_joiner': {'bert_dim': 768, 'out_dim': 768},
           'text_decoder': {'hidden_dim': 768, 'dropout': 0.1, 'nheads': 8, 'pos_enc': False, 'num_layers': 3},
           'co_att': {'visualization': False,
                      'bi_num_attention_heads': 16,
                      'bi_hidden_size': 768,
                      'hidden_size': 768,
                      'intermediate_size': 3072,
                      'output_size': 768,
                      'attention_probs_dropout_prob': 0.1,
                      'hidden_dropout_prob': 0.1,
                      'hidden_act': 'gelu',
                      'v_hidden_size': 768,
                      'v_intermediate_size': 3072,
                      'v_output_size': 768,
                      'v_attention_probs_dropout_prob': 0.1,
                      'v_hidden_dropout_prob': 0.1,
                      'v_hidden_act': 'gelu',
                      'num_layers': 3},
           'losses': {'CaptionLoss': {'name': 'caption_criterion', 'pad_idx': None, 'loss_wts': {'loss_caption': 0.05}},
                      'VqaLoss': {'name': 'vqa_criterion', 'pad_idx': None, 'loss_wts': {'loss_vqa': 1}},
                      'ClsLoss': {'name': 'cls_criterion', 'pad_idx': None, 'loss_wts': {'loss_cls': 1}},
                      'Localization': {'name': 'localization_criterion',
                                       'cost_wts': {'ce': 1, 'bbox': 5, 'giou': 2},
                                       'loss_wts': {'loss_ce': 1, 'loss_bbox': 5, 'loss_giou': 2},
                                       'eos_coef': 0.1,
                                       'num_classes': 1}}},
 'training': {'ckpt': None,
              'freeze': False,
              'frozen_epochs': 10,
              'frozen_batch_size': 120,
              'num_epochs': 40,
              'batch_size': 120,
              'num_workers': 30,
              'data_source': 'synthetic',          # 'files': CocoMultitaskDataset(learning_datasets, task_configs) behind a DeviceLoader
              'prefetch': 1,                       # batches the loader's worker thread prepares ahead (data_source: files)
              'vis_step': 2000,
              'visualize': 'off',                  # 'device': training visualisations every vis_step steps (gpv1_amd.visualize)
              'vis_labels': False,                 # scores above the predicted boxes, `GT` below the ground truth (visualize(labels=True))
              'log_step': 10,
              'ckpt_step': 2000,
              'lr': 0.0001,
              'lr_backbone': 1e-05,
              'weight_decay': 0.0001,
              'lr_milestones': [10, 15, 20, 25, 30, 35],
              'lr_drop': 0.5,
              'lr_warmup': True,
              'lr_linear_decay': True,
              'lr_warmup_fraction': 0.1,
              'clip_max_norm': 0.1,
              'run_vis_at_launch': True,
              'num_vis_samples': 15,
              'run_eval_at_launch': True,
              'num_val_samples': {'coco_vqa': 20000, 'coco_cap': 10000, 'coco_det': 10000, 'coco_cls': 10000, 'refcocop': 2000}},
 'eval': {'task': 'CocoVqa',
          'ckpt': '${exp_dir}/ckpts/model.pth',
          'batch_size': 20,
          'num_workers': 20,
          'subset': 'val',
          'predict': True,
          'num_output_boxes': 5,
          'beam_size': 5}}


# configs/task/coco_learning_tasks.yaml (`# @package task_configs`): where the preprocessed sample files and the images lie.
# Settings only; gpv1_amd.datasets reads them.
def _task(samples, subsets=('train', 'val', 'test'), **more):
    return dict({'image_dir': '${task_configs.image_dir}', 'image_size': '${task_configs.image_size}', 'read_image': '${task_configs.read_image}'},
                **more, samples={s: samples.replace('SUBSET', s) for s in subsets}, max_samples={s: None for s in subsets})


_LPD = '${data_dir}/learning_phase_data'
_TREE['task_configs'] = {
    'image_dir': _LPD + '/coco/images',
    'image_size': {'H': 480, 'W': 640},
    'read_image': True,
    'data_split': 'gpv_split',
    'coco_captioning': _task(_LPD + '/coco_captions/${task_configs.data_split}/SUBSET.json'),
    'coco_detection': _task(_LPD + '/coco_detection/${task_configs.data_split}/SUBSET.json'),
    'coco_classification': _task(_LPD + '/coco_classification/${task_configs.data_split}/SUBSET.json'),
    'coco_vqa': _task(_LPD + '/vqa/${task_configs.data_split}/SUBSET.json', subsets=('train', 'val', 'test', 'testdev')),
    'refcocop': _task(_LPD + '/refcocop/SUBSET.json', train_percent=100)}
_TREE['task_configs']['refcocop']['samples']['train'] = _LPD + '/refcocop/train_${task_configs.refcocop.train_percent}.json'

# configs/learning_datasets/*.yaml: the task mixes `learning_datasets=<name>` selects (scripts/train.sh:14-34); `vqa` is the
# default of configs/exp/gpv.yaml:25
_TASKS = {'cap': ('CocoCaptioning', 'coco_captioning', 'coco_cap'), 'det': ('CocoDetection', 'coco_detection', 'coco_det'),
          'cls': ('CocoClassification', 'coco_classification', 'coco_cls'), 'vqa': ('CocoVqa', 'coco_vqa', 'coco_vqa'),
          'refcocop': ('RefCocop', 'refcocop', 'refcocop')}
_MIXES = {'all': ('cap', 'det', 'cls', 'vqa'), 'cap': ('cap',), 'cap_vqa': ('cap', 'vqa'), 'cls': ('cls',), 'det': ('det',),
          'det_cap': ('cap', 'det'), 'det_cls': ('det', 'cls'), 'det_vqa': ('det', 'vqa'), 'det_vqa_cap': ('det', 'vqa', 'cap'),
          'refcocop': ('refcocop',), 'vqa': ('vqa',)}
GROUP_OPTIONS = {'learning_datasets': {mix: {_TASKS[t][0]: {'task_config': _TASKS[t][1], 'name': _TASKS[t][2]} for t in ts}
                                       for mix, ts in _MIXES.items()}}
_TREE['learning_datasets'] = copy.deepcopy(GROUP_OPTIONS['learning_datasets']['vqa'])


def default_tree():
    return copy.deepcopy(_TREE)
