// The fused deep-supervision losses (loss.hip): CE + Dice and the focal forms, forward and backward.
#pragma once
#include "hdf_common.h"

// class slots the loss, metric, staging and inference-tail kernels hold in registers: fixes the [B, 8, 3] Dice counts and
// the 8 x 8 confusion matrix of the ABI
constexpr int HDF_CLASS_SLOTS = 8;

struct LossScales {
  float V[4];
  float weight[4];
  int blocks[4];  // partial rows written per (scale, sample)
};

int hdf_loss_blocks();
size_t hdf_loss_workspace_floats(int N, int nscale);
int hdf_launch_loss_fwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                        int H, int W, float* ws, float* loss_out, hipStream_t st, float w_ce = 1.f, float w_dice = 1.f,
                        const float* class_weight = nullptr, int dice_ignore = 0);
int hdf_launch_loss_bwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                        int H, int W, const float* ws, const float* grad_out, void* const* dlogits, hipStream_t st,
                        float w_ce = 1.f, float w_dice = 1.f, const float* class_weight = nullptr, int dice_ignore = 0);
// focal forms (FocalLoss / FLPlusDice): w_focal * focal + w_dice * Dice per scale; reduction 0 sum, 1 mean
int hdf_launch_loss_focal_fwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                              int H, int W, float* ws, float* loss_out, hipStream_t st, float w_focal, float alpha,
                              float gamma, int reduction, float w_dice, const float* class_weight, int dice_ignore);
int hdf_launch_loss_focal_bwd(int dtype, const void* const* logits, const float* target, int nscale, int N, int C, int D,
                              int H, int W, const float* ws, const float* grad_out, void* const* dlogits,
                              hipStream_t st, float w_focal, float alpha, float gamma, int reduction, float w_dice,
                              const float* class_weight, int dice_ignore);
