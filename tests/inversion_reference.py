"""Stock-torch restatement of train_inversion (lora_diffusion/cli_lora_pti.py:290-346) with loss_step (:170-247), fp32, on any
device: AdamW over the WHOLE token table (:651-657), the LambdaLR stepped first (:293), accumulation (:299-313), clip_ti_decay
(:318-336) and the restore of every other row from a clone (:280,344-346).  The yardstick of diffusion_finetuning_amd.inversion
(tests/test_gpu_inversion.py) and the stock run of tools/inversion_step_time.py."""
import torch
import torch.nn.functional as F


def reference_inversion(unet, text_encoder, placeholder_ids, batches, lr, weight_decay, accum_iter, sched_lambda,
                        clip_ti_decay, v_prediction, sqrt_acp, sqrt_1macp, on_step=None):
    """batches: [(latents, noise, timesteps, input_ids, raw mask | None)] on the models' device.  Updates the token table in
    place; returns (losses [micro-steps], learning rates [micro-steps]).  on_step(g): called after every micro-step."""
    table = text_encoder.get_input_embeddings().weight
    V = table.shape[0]
    index_no_updates = torch.ones(V, dtype=torch.bool, device=table.device)
    index_no_updates[list(placeholder_ids)] = False
    index_updates = ~index_no_updates
    orig_embeds_params = table.data.clone()
    optimizer = torch.optim.AdamW([table], lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=weight_decay)
    lr_scheduler = torch.optim.lr_scheduler.LambdaLR(optimizer, sched_lambda)
    losses, lrs = [], []
    for g, (latents, noise, timesteps, ids, mask) in enumerate(batches):
        lr_scheduler.step()
        a = sqrt_acp[timesteps].view(-1, 1, 1, 1)
        s = sqrt_1macp[timesteps].view(-1, 1, 1, 1)
        noisy = a * latents + s * noise  # DDPMScheduler.add_noise
        ehs = text_encoder(ids)[0]
        pred = unet(noisy, timesteps, ehs).sample
        target = a * noise - s * latents if v_prediction else noise  # get_velocity | epsilon
        if mask is not None:
            m = mask.reshape(pred.shape[0], 1, pred.shape[2] * 8, pred.shape[3] * 8)
            m = F.interpolate(m.float(), size=pred.shape[-2:], mode="nearest") + 0.05
            m = m / m.mean()
            pred, target = pred * m, target * m
        loss = F.mse_loss(pred.float(), target.float(), reduction="mean") / accum_iter
        loss.backward()
        losses.append(loss.detach().reshape(()))
        lrs.append(lr_scheduler.get_last_lr()[0])
        if g % accum_iter == 0:
            optimizer.step()
            optimizer.zero_grad()
            with torch.no_grad():
                if clip_ti_decay:
                    pre_norm = table[index_updates, :].norm(dim=-1, keepdim=True)
                    lambda_ = min(1.0, 100 * lr_scheduler.get_last_lr()[0])
                    table[index_updates] = F.normalize(table[index_updates, :], dim=-1) * (pre_norm + lambda_ * (0.4 - pre_norm))
                table[index_no_updates] = orig_embeds_params[index_no_updates]
        if on_step is not None:
            on_step(g)
    table.grad = None
    return torch.stack(losses), lrs


def config5_models(device, dtype=torch.float32):
    """BASELINE config 5's models at full size, as train_inversion sees them: an SD2.1-768-shaped UNet (the build's harness,
    random init, frozen, no LoRA yet — injection comes after inversion, :693) and an OpenCLIP-H-shaped text encoder (hidden
    1024, 23 layers, 16 heads; bench.py's "openclip-h-ti") frozen except its 49408 × 1024 fp32 token table (:638-647)."""
    from transformers import CLIPTextConfig, CLIPTextModel

    from harness.unet import UNet2DConditionModel, sd21_768_config

    torch.manual_seed(0)
    with torch.device(device):
        unet = UNet2DConditionModel(sd21_768_config())
    unet = unet.to(dtype)
    unet.requires_grad_(False)
    torch.manual_seed(2)
    te = CLIPTextModel(CLIPTextConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=23, num_attention_heads=16,
                                      vocab_size=49408, max_position_embeddings=77, bos_token_id=49406, eos_token_id=49407,
                                      pad_token_id=0, hidden_act="gelu"))
    te.requires_grad_(False)
    te = te.to(device).to(dtype)
    te.get_input_embeddings().float().weight.requires_grad_(True)
    return unet, te


def config5_batches(n, device, placeholder_ids, latent=96, seed_base=1000):
    """n micro-batches of batch 1: latents, noise, t < 1000 (t_mutliplier 1 in this phase), caption-shaped ids holding the
    placeholder tokens ("a photo of <s1><s2>"), no mask."""
    out = []
    for s in range(n):
        g = torch.Generator().manual_seed(seed_base + s)
        lat = torch.randn(1, 4, latent, latent, generator=g) * 0.18215
        noise = torch.randn(1, 4, latent, latent, generator=g)
        t = torch.randint(0, 1000, (1,), generator=g)
        ids = torch.randint(2, 49000, (1, 77), generator=g)
        ids[:, 0], ids[:, 6:] = 49406, 49407
        ids[0, 4:4 + len(placeholder_ids)] = torch.tensor(list(placeholder_ids))
        out.append((lat.to(device), noise.to(device), t.to(device), ids.to(device), None))
    return out
