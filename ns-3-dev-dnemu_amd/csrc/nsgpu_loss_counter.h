// nsgpu_loss_counter.h — PacketLossCounter (packet-loss-counter.cc:32-120), restated literally as one function
// the host and the device share: UdpServer::HandleRead's NotifyReceived (seq) on a nsgpu_loss_counter.
#pragma once
#include "nsgpu_types.h"

// SetBitMapSize (:53-64): window / 8 bytes, all 0xFF.
NSGPU_HD static inline void nsgpu_loss_counter_init(nsgpu_loss_counter *c, uint32_t window) {
  c->lost = 0;
  c->last_max_seq = 0;
  c->window = window;
  c->received = 0;
  for (uint32_t i = 0; i < NSGPU_LOSS_WINDOW_MAX / 8; i++) c->map[i] = 0xFF;
}
// GetBit (:72-76), SetBit (:78-89): byte (seq % window) / 8, bit 7 - seq % 8.
NSGPU_HD static inline uint32_t nsgpu_loss_counter_get(const nsgpu_loss_counter *c, uint32_t seq) {
  return (c->map[(seq % c->window) / 8] >> (7 - (seq % 8))) & 0x01u;
}
NSGPU_HD static inline void nsgpu_loss_counter_set(nsgpu_loss_counter *c, uint32_t seq, bool val) {
  if (val) c->map[(seq % c->window) / 8] |= (uint8_t)(0x80u >> (seq % 8));
  else c->map[(seq % c->window) / 8] &= (uint8_t)~(0x80u >> (seq % 8));
}
// NotifyReceived (:103-120): for (i = last + 1; i <= seq; i++) { if (!GetBit (i)) lost++; SetBit (i, 0); } —
// with its quirks: a lost sequence number 0 is never counted (the loop starts at 1), a loss is counted only
// when the window passes it.  The loop visits the bits cyclically, so after `window` iterations every bit it
// reads is one it has just cleared: each further iteration adds exactly one loss and changes nothing.  The
// first min (gap, window) iterations run as written and the other gap - window are added at once (a gap of
// 10^6 costs `window` iterations; the reference's loop would not end for seq = 0xffffffff).
NSGPU_HD static inline void nsgpu_loss_counter_notify(nsgpu_loss_counter *c, uint32_t seq) {
  if (seq > c->last_max_seq) {
    const uint32_t gap = seq - c->last_max_seq;
    const uint32_t n = gap < c->window ? gap : c->window;
    for (uint32_t k = 1; k <= n; k++) {
      const uint32_t i = c->last_max_seq + k;
      if (nsgpu_loss_counter_get(c, i) != 1) c->lost++;
      nsgpu_loss_counter_set(c, i, false);
    }
    c->lost += gap - n;
  }
  nsgpu_loss_counter_set(c, seq, true);
  if (seq > c->last_max_seq) c->last_max_seq = seq;
}
